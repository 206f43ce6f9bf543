"""Replays one row of tests/golden/cconv_dispatch.json on a loaded libdmcf_hip.so: the three host-side queries of the forward
CConv dispatch (dmcf_cconv_kernel_name, dmcf_cconv_extents_kernel_name, dmcf_cconv_workspace_bytes).  None of them launches or
touches a device: the pointers are only tested for NULL and alignment.  Shared by tests/golden/make_cconv_dispatch.py, which
records the rows on a build of the parent commit, and tests/test_cconv_dispatch_snapshot.py, which holds the tree to them."""
import ctypes
import os

from dmcf_amd import _lib, ops

# a row's inputs, in file order
INPUTS = ("d0", "d1", "d2", "cin", "cout", "sym_axis", "hint", "flags", "mapping", "interp", "kind", "misaligned", "n_inp", "n_out",
          "split", "kernel")
# ... and what the parent answered: return code and index into the file's "names" of both name queries, the workspace bytes
OUTPUTS = ("name_rc", "name", "ext_rc", "ext_name", "workspace_bytes")

KINDS = ("plain", "values", "importance")  # poly6 on re-formed distances | an explicit value per pair | poly6 + per-point importance
FAKE = 1 << 20  # a 16-byte aligned non-NULL "pointer"


def args_of(row):
    """CconvArgs of a row (a dict over INPUTS)."""
    a = _lib.CconvArgs()
    for d, k in enumerate(("d0", "d1", "d2", "cin", "cout")):
        a.filter_dims[d] = row[k]
    sym = row["sym_axis"] >= 0
    a.sym_axis = row["sym_axis"] if sym else 0
    a.n_out, a.n_inp, a.n_pairs = row["n_out"], row["n_inp"], 10000
    a.filters = a.out_positions = a.inp_positions = a.neighbors_index = a.neighbors_row_splits = a.out = FAKE
    a.inp_features = FAKE + (4 if row["misaligned"] else 0)
    kind = KINDS[row["kind"]]
    a.inp_importance = FAKE if kind == "importance" else None
    a.neighbors_value = FAKE if kind == "values" else None
    a.window = ops.WINDOWS["explicit" if kind == "values" else "poly6"]
    a.extent, a.window_fac = 0.46, 1.0
    a.coordinate_mapping, a.interpolation = row["mapping"], row["interp"]
    a.flags = row["flags"] | (ops.FLAG_SYMMETRIC if sym else 0)
    a.row_length_hint = row["hint"]
    return a


def query(L, row, setenv, delenv):
    """The row's OUTPUTS from library L, names as strings (None where the call returned an error).  setenv(name, value) /
    delenv(name): how the caller wants the environment changed (a test passes monkeypatch's)."""
    for var, value in (("DMCF_CCONV_KERNEL", row["kernel"]), ("DMCF_MFMA_SPLIT", "1" if row["split"] else None)):
        if value is None:
            delenv(var)
        else:
            setenv(var, value)
    a = args_of(row)
    out = []
    for fn in (L.dmcf_cconv_kernel_name, L.dmcf_cconv_extents_kernel_name):
        buf = ctypes.create_string_buffer(96)
        rc = fn(ctypes.byref(a), buf, 96)
        out += [rc, buf.value.decode() if rc == 0 else None]
    out.append(int(L.dmcf_cconv_workspace_bytes(ctypes.byref(a))))
    return out


def environ_set(name, value):
    os.environ[name] = value


def environ_del(name):
    os.environ.pop(name, None)
