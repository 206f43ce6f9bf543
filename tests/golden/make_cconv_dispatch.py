"""Generates tests/golden/cconv_dispatch.json: what the forward CConv dispatch of a REFERENCE COMMIT answers on a grid of
arguments -- return code and string of dmcf_cconv_kernel_name / dmcf_cconv_extents_kernel_name and the value of
dmcf_cconv_workspace_bytes (no GPU needed: tests/cconv_dispatch_ref.py).  tests/test_cconv_dispatch_snapshot.py holds the
tree to the file, so a change of the dispatch's host code shows as a diff of named rows.

    python tests/golden/make_cconv_dispatch.py --rev <commit>     # default HEAD^: the parent of the commit under test

exports that commit into a temporary directory, builds its libdmcf_hip.so there (make -C dmcf_amd/csrc; needs hipcc) and
queries it.  --lib <path> queries an already built library of that commit instead.

The grid is a thinned product (the file stays under ~200 KB) that keeps every value of every axis:
  A  every filter shape x cin x cout, nothing forced, the row-length hint cycling
  B  the shapes the specialised forms take x every DMCF_CCONV_KERNEL value x cin, cout cycling
  C  around base layers that reach every form: one axis at a time (hint, each flag, mapping, interpolation, align, layer
     kind, feature alignment, n_inp, n_out x DMCF_MFMA_SPLIT), unforced and under three of the ten DMCF_CCONV_KERNEL values
     (rotating over the bases)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cconv_dispatch_ref as dr  # noqa: E402
from dmcf_amd import _lib, ops  # noqa: E402

OUT = os.path.join(HERE, "cconv_dispatch.json")

SHAPES = [((4, 4, 4), -1), ((1, 8, 8), -1), ((1, 8, 1), -1), ((3, 5, 2), -1), ((6, 6, 6), -1), ((4, 4, 2), 2), ((6, 3, 6), 1)]
CINS = [1, 3, 4, 8, 12, 16, 17, 24, 32, 36]
COUTS = [1, 3, 4, 16, 17, 32, 33, 64, 65]
KERNELS = [None, "lds", "mfma", "blk", "cls", "z3", "pair", "ws", "g16", "direct", "bogus"]
N_INPS = [2420, 1 << 24, 15_000_000]  # (the last: n_inp * cin * 4 >= 2^31 at 36 channels)
N_OUTS = [100, 16384, 20000]
ALIGN = ops.FLAG_ALIGN_CORNERS
DEFAULT = dict(sym_axis=-1, hint=0, flags=ALIGN, mapping=ops.MAPPINGS["ball_to_cube_volume_preserving"],
               interp=ops.INTERPOLATIONS["linear"], kind=0, misaligned=0, n_inp=2420, n_out=100, split=0, kernel=None)
# (shape, sym_axis, cin, cout): between them, unforced or forced, they reach all nine kernel families
BASES = [((4, 4, 4), -1, 32, 32), ((4, 4, 4), -1, 24, 4), ((4, 4, 4), -1, 16, 16), ((4, 4, 4), -1, 8, 64), ((4, 4, 4), -1, 4, 32),
         ((4, 4, 4), -1, 36, 3), ((4, 4, 4), -1, 12, 65), ((4, 4, 2), 2, 16, 3), ((1, 8, 8), -1, 32, 32), ((1, 8, 8), -1, 17, 4),
         ((3, 5, 2), -1, 24, 17), ((6, 6, 6), -1, 32, 3), ((6, 3, 6), 1, 32, 3), ((6, 3, 6), 1, 8, 1), ((1, 8, 1), -1, 3, 1)]


def rows():
    out, seen = [], set()

    def add(shape, cin, cout, **kw):
        r = dict(DEFAULT, d0=shape[0], d1=shape[1], d2=shape[2], cin=cin, cout=cout, **kw)
        key = tuple(r[k] for k in dr.INPUTS)
        if key not in seen:
            seen.add(key)
            out.append(r)

    n = 0
    for shape, sym in SHAPES:  # A
        for cin in CINS:
            for cout in COUTS:
                add(shape, cin, cout, sym_axis=sym, hint=n % 3)
                n += 1
    for shape, sym in (SHAPES[0], SHAPES[5], SHAPES[4], SHAPES[1]):  # B
        for kernel in KERNELS[1:]:
            for cin in CINS:
                for j in range(2):
                    add(shape, cin, COUTS[(n + 4 * j) % len(COUTS)], sym_axis=sym, kernel=kernel, hint=n % 3)
                n += 1
    for b, (shape, sym, cin, cout) in enumerate(BASES):  # C
        for kernel in [None] + [KERNELS[1 + (3 * b + j) % 10] for j in range(3)]:  # (every value: 15 bases x 3 of the 10)
            def var(**kw):
                add(shape, cin, cout, sym_axis=sym, kernel=kernel, **kw)
            for hint in (0, 1, 2):
                var(hint=hint)
            for flag in (ops.FLAG_NORMALIZE, ops.FLAG_SKIP_SELF, ops.FLAG_ACCUMULATE):
                var(flags=ALIGN | flag)
            var(flags=0)
            for m in ops.MAPPINGS.values():
                var(mapping=m)
            for i in ops.INTERPOLATIONS.values():
                var(interp=i)
            for kind in (1, 2):
                var(kind=kind, hint=2)
            var(misaligned=1)
            for n_inp in N_INPS:
                var(n_inp=n_inp)
            for n_out in N_OUTS:
                for split in (0, 1):
                    var(n_out=n_out, split=split)
    return out


def build_reference(rev, tmp):
    """The library of commit `rev`, built in an export of it under tmp."""
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
    subprocess.run(["make", "-C", os.path.join(tmp, "dmcf_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    return os.path.join(tmp, "dmcf_amd", "libdmcf_hip.so")


def load(path):
    L = ctypes.CDLL(path)
    for fn in (L.dmcf_cconv_kernel_name, L.dmcf_cconv_extents_kernel_name):
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(_lib.CconvArgs), ctypes.c_char_p, ctypes.c_size_t]
    L.dmcf_cconv_workspace_bytes.restype, L.dmcf_cconv_workspace_bytes.argtypes = ctypes.c_size_t, [ctypes.POINTER(_lib.CconvArgs)]
    return L


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD^")
    ap.add_argument("--lib", default=None)
    opt = ap.parse_args()
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", opt.rev], check=True, capture_output=True, text=True).stdout.strip()
    with tempfile.TemporaryDirectory() as tmp:
        L = load(opt.lib or build_reference(rev, tmp))
        names, table = [], []
        for r in rows():
            rc, name, erc, ename, ws = dr.query(L, r, dr.environ_set, dr.environ_del)
            for s in (name, ename):
                if s is not None and s not in names:
                    names.append(s)
            table.append([r[k] for k in dr.INPUTS] + [rc, names.index(name) if name is not None else -1, erc,
                                                      names.index(ename) if ename is not None else -1, ws])
    with open(OUT, "w") as f:
        f.write('{"commit": "%s",\n "columns": %s,\n "names": %s,\n "rows": [\n' % (rev, json.dumps(dr.INPUTS + dr.OUTPUTS), json.dumps(names)))
        f.write(",\n".join(json.dumps(t, separators=(",", ":")) for t in table))
        f.write("\n]}\n")
    print(f"{len(table)} rows, {len(names)} kernel names, {os.path.getsize(OUT)} bytes -> {OUT}")
