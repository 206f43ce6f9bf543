"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/dmcf_hip.h declares (no compute calls -- there is no GPU here), and the ctypes binding of dmcf_amd/_lib.py -- PROTOTYPES,
the struct mirrors, the mirrored constants -- says what the header says (parsed here; needs neither the library nor a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dmcf_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(hip_lib):
    from dmcf_amd import _lib
    declared = _declared_symbols()
    assert declared, "no prototypes found in include/dmcf_hip.h"
    assert sorted(_lib.SYMBOLS) == declared
    for name in declared:
        assert hasattr(hip_lib, name), f"{name} declared in dmcf_hip.h but not exported"


def test_version_and_error_strings(hip_lib):
    assert hip_lib.dmcf_version() >= 100
    assert hip_lib.dmcf_error_string(0) == b"ok"
    assert b"workspace" in hip_lib.dmcf_error_string(-2)


def test_workspace_queries_and_host_validation(hip_lib):
    # host-side argument validation runs without a device
    assert hip_lib.dmcf_frs_workspace_bytes(1000, 1000) > 1000 * 16
    assert hip_lib.dmcf_frs_workspace_bytes(-1, 0) == 0
    assert hip_lib.dmcf_frs_build(None, 10, 0.1, None, 0, None) == -1  # null workspace -> DMCF_EINVAL
    assert hip_lib.dmcf_reduce_subarrays_sum(None, None, -1, None, None) == -1
    assert hip_lib.dmcf_points_aabb_workspace_bytes() >= 6 * 4
    assert hip_lib.dmcf_dense_forward(None, 10, 8, None, 16, None, None, None, None) == -1  # null operands -> DMCF_EINVAL
    assert hip_lib.dmcf_points_aabb(None, 10, None, None, 0, None) == -1  # no output -> DMCF_EINVAL
    from dmcf_amd._lib import CconvArgs
    a = CconvArgs()
    assert hip_lib.dmcf_cconv_forward(ctypes.byref(a), None, 0, None) == -1  # zero filter dims


def test_grid_pos_refuses_more_than_2_32_candidates(hip_lib):
    """Candidate ranks are 32-bit: 2 n n_off >= 2^32 is DMCF_EUNSUPPORTED from every grid_pos entry point, before anything is
    enqueued.  Counts only: n = 400000 at pad = 8 (18^3 offsets) is 4.67e9 candidates; the workspace has the right size and
    nothing in it or in the positions is touched (a word each would do: the call returns from its argument checks)."""
    import torch
    L = hip_lib
    n, pad = 400000, 8
    assert 2 * n * 18 ** 3 >= 1 << 32
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    nb = L.dmcf_grid_pos_workspace_bytes(n)
    nbb = L.dmcf_grid_pos_workspace_bytes_batched(n, 2)
    assert 0 < nb < 64 << 20 and 0 < nbb < 64 << 20  # (rows, not candidates: tens of megabytes)
    buf = torch.zeros(max(nb, nbb) + 256, dtype=torch.uint8, device=dev)
    ws = (buf.data_ptr() + 255) // 256 * 256
    pos = torch.zeros(16, dtype=torch.float32, device=dev).data_ptr()
    rs = torch.tensor([0, n // 2, n], dtype=torch.int64, device=dev).data_ptr()
    vs = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
    EUNSUPPORTED = -4
    assert L.dmcf_grid_pos_bounds(pos, n, vs, 1, None, pad, 0.1, ws, nb, None) == EUNSUPPORTED
    assert L.dmcf_grid_pos_count(pos, n, vs, 1, pad, 0.1, ws, nb, pos, 4, None) == EUNSUPPORTED
    assert L.dmcf_grid_pos_write(pos, n, vs, 1, pad, 0.1, ws, nb, pos, 4, pos, 1, None) == EUNSUPPORTED
    assert L.dmcf_grid_pos_bounds_batched(pos, n, rs, 2, vs, 1, None, pad, 0.1, ws, nbb, None) == EUNSUPPORTED
    assert L.dmcf_grid_pos_count_batched(pos, n, rs, 2, vs, 1, pad, 0.1, ws, nbb, pos, 4, rs, None) == EUNSUPPORTED
    assert L.dmcf_grid_pos_write_batched(pos, n, rs, 2, vs, 1, pad, 0.1, ws, nbb, pos, 4, pos, 1, None) == EUNSUPPORTED
    # just under the limit the same arguments pass that check: the next one (no workspace) answers
    under = ((1 << 32) - 2) // (2 * 18 ** 3)
    assert 2 * under * 18 ** 3 < (1 << 32) - 1 <= 2 * (under + 1) * 18 ** 3
    assert L.dmcf_grid_pos_bounds(pos, under, vs, 1, None, pad, 0.1, None, 0, None) == -1
    assert L.dmcf_grid_pos_bounds(pos, under + 1, vs, 1, None, pad, 0.1, None, 0, None) == EUNSUPPORTED
    # the fewer offsets of a 2-D lattice move the limit: 18^2 offsets at the same n are fine
    flat = (ctypes.c_float * 3)(0.1, 0.1, 0.0)
    assert L.dmcf_grid_pos_bounds(pos, n, flat, 1, None, pad, 0.1, None, 0, None) == -1


# ---- the binding (dmcf_amd/_lib.py: the struct mirrors and PROTOTYPES) against include/dmcf_hip.h -------------------------------
# The header is plain C and regular: comments are stripped and regular expressions do the rest.  A parsed declaration is a
# tuple (name, C base type, is_pointer, array length or None); a function's name is that of the parameter (None if unnamed).

C_TO_CTYPES = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
    "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "dmcf_stream_t": ctypes.c_void_p,
}


def _header_text():
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _parse_declaration(text):
    """'const float* a', 'int32_t b[3], c[3]' or 'size_t' -> [(name, base type, is_pointer, array length)]."""
    m = re.fullmatch(r"\s*(?:const\s+)?(?:struct\s+)?(\w+)\s*(\*?)\s*(.*?)\s*", text, flags=re.S)
    assert m, text
    base, star, rest = m.groups()
    out = []
    for d in rest.split(","):
        dm = re.fullmatch(r"\s*(\*?)\s*(\w*)\s*(?:\[(\d+)\])?\s*", d)
        assert dm, text
        out.append((dm.group(2) or None, base, bool(star or dm.group(1)), int(dm.group(3)) if dm.group(3) else None))
    return out


def _header_structs():
    """{struct name: [field declarations]} in the header's order."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(dmcf_\w+)\s*\{(.*?)\}\s*\1\s*;", _header_text(), flags=re.S):
        out[name] = [f for line in body.split(";") if line.strip() for f in _parse_declaration(line)]
    return out


def _header_prototypes():
    """{function name: (return declaration, [parameter declarations])} in the header's order."""
    text = re.sub(r"\{[^{}]*\}", "", _header_text())  # struct and enum bodies
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\b(dmcf_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() == "void" else [_parse_declaration(p)[0] for p in params.split(",")]
        out[name] = (_parse_declaration(ret)[0], params)
    return out


def _header_constants():
    """{name: value} of the integer #defines and of every enum member."""
    text = _header_text()
    out = {n: int(v) for n, v in re.findall(r"^#define\s+(DMCF_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s+dmcf_\w+\s*\{(.*?)\}", text, flags=re.S):
        out.update({n: int(v) for n, v in re.findall(r"(DMCF_\w+)\s*=\s*(-?\d+)", body)})
    return out


def _struct_mirrors():
    """{struct name: ctypes.Structure subclass of dmcf_amd._lib}, found through the 'struct dmcf_...' of the class's docstring."""
    from dmcf_amd import _lib
    out = {}
    for cls in vars(_lib).values():
        if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
            m = re.search(r"\bstruct (dmcf_\w+)", cls.__doc__ or "")
            assert m, f"{cls.__name__}: the docstring does not name the struct it mirrors"
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = cls
    return out


def _type_mismatch(decl, ctype, mirrors, is_return=False):
    """None if `ctype` is what the table above maps the C declaration to, else what is wrong."""
    _, base, pointer, length = decl
    if length is not None:
        if not (isinstance(ctype, type) and issubclass(ctype, ctypes.Array)):
            return f"{base}[{length}] bound as {ctype}"
        if ctype._length_ != length:
            return f"{base}[{length}] bound with length {ctype._length_}"
        ctype = ctype._type_
    if not pointer:
        want = C_TO_CTYPES.get(base)
        return None if want is not None and ctype is want else f"{base} bound as {ctype}"
    if is_return:
        return None if base == "char" and ctype is ctypes.c_char_p else f"{base}* returned as {ctype}"
    if ctype in (ctypes.c_void_p, ctypes.c_char_p):
        return None
    if not (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer)):
        return f"{base}* bound as {ctype}"
    want = mirrors.get(base, C_TO_CTYPES.get(base))
    return None if ctype._type_ is want else f"{base}* bound as a pointer to {ctype._type_}"


def _binding_mismatches(structs, prototypes, mirrors, fields, bound):
    """Everything in which the binding differs from the header.  structs / prototypes: the parsed header; mirrors: the
    Structure classes by struct name; fields: their _fields_ lists by struct name; bound: PROTOTYPES."""
    bad = []
    for s in sorted(set(structs) | set(fields)):
        if s not in structs or s not in fields:
            bad.append(f"struct {s}: " + ("no mirror" if s in structs else "not in the header"))
            continue
        if [f[0] for f in structs[s]] != [f[0] for f in fields[s]]:
            bad.append(f"struct {s}: fields {[f[0] for f in fields[s]]}, the header has {[f[0] for f in structs[s]]}")
            continue
        for decl, (fname, ctype) in zip(structs[s], fields[s]):
            why = _type_mismatch(decl, ctype, mirrors)
            if why:
                bad.append(f"struct {s}.{fname}: {why}")
    for f in sorted(set(prototypes) | set(bound)):
        if f not in prototypes or f not in bound:
            bad.append(f"{f}: " + ("no PROTOTYPES row" if f in prototypes else "not in the header"))
            continue
        (ret, params), (restype, argtypes) = prototypes[f], bound[f]
        why = _type_mismatch(ret, restype, mirrors, is_return=True)
        if why:
            bad.append(f"{f}: return {why}")
        if len(params) != len(argtypes):
            bad.append(f"{f}: {len(argtypes)} argtypes, the header has {len(params)} parameters")
            continue
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            why = _type_mismatch(decl, ctype, mirrors)
            if why:
                bad.append(f"{f}: parameter {k} ({decl[0]}): {why}")
    return bad


@pytest.fixture(scope="module")
def binding():
    """(structs, prototypes, mirrors, fields, bound): the parsed header and the binding, as _binding_mismatches takes them."""
    from dmcf_amd import _lib
    mirrors = _struct_mirrors()
    return (_header_structs(), _header_prototypes(), mirrors, {s: list(c._fields_) for s, c in mirrors.items()},
            dict(_lib.PROTOTYPES))


def test_header_parse_is_complete(binding):
    """The two checks below cannot pass on a header the parser read only in part, or on a mirror it did not find."""
    from dmcf_amd import _lib
    structs, prototypes, mirrors, _, _ = binding
    assert sorted(prototypes) == _declared_symbols() and len(prototypes) > 100
    assert len(structs) == len(re.findall(r"typedef\s+struct\s+dmcf_", _header_text())) >= 14
    assert sorted(mirrors) == sorted(structs)
    classes = [c for c in vars(_lib).values()
               if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    assert sorted(classes, key=id) == sorted(mirrors.values(), key=id)
    # multi-declarator lines and arrays
    lattice = {f[0]: f for f in structs["dmcf_lattice_conv_args"]}
    assert lattice["base_min"] == ("base_min", "int32_t", False, 3) and lattice["base_dims"] == ("base_dims", "int32_t", False, 3)
    assert prototypes["dmcf_version"] == ((None, "int", False, None), [])
    assert prototypes["dmcf_error_string"] == ((None, "char", True, None), [("code", "int", False, None)])


def test_struct_layout_matches_header(binding):
    """Field names, order, scalar types and array lengths of all the ctypes mirrors equal the header's: ctypes lays out naturally
    aligned fields as the C compiler does, so that is the layout."""
    from dmcf_amd._lib import CconvArgs
    structs, _, mirrors, fields, _ = binding
    assert mirrors["dmcf_cconv_args"] is CconvArgs
    assert [f[0] for f in structs["dmcf_cconv_args"]] == [f[0] for f in CconvArgs._fields_]
    assert _binding_mismatches(structs, {}, mirrors, fields, {}) == []


def test_prototypes_match_header(binding):
    """PROTOTYPES has, for every function of the header, the mapped return type and the mapped type of every parameter."""
    from dmcf_amd import _lib
    structs, prototypes, mirrors, fields, bound = binding
    assert list(bound) == list(prototypes), "PROTOTYPES is not in the header's order"
    assert _lib.SYMBOLS == list(prototypes)
    assert _binding_mismatches(structs, prototypes, mirrors, fields, bound) == []


def test_binding_check_reports_alterations(binding):
    """The comparison, on altered COPIES of the binding, reports each alteration (and nothing else)."""
    structs, prototypes, mirrors, fields, bound = binding

    def mismatches(fields=fields, bound=bound):
        return _binding_mismatches(structs, prototypes, mirrors, fields, bound)

    def with_args(name, argtypes):
        return {**bound, name: (bound[name][0], tuple(argtypes))}

    assert mismatches() == []
    # one c_int64 turned into c_int32
    args = list(bound["dmcf_frs_build"][1])
    assert args[1] is ctypes.c_int64
    args[1] = ctypes.c_int32
    bad = mismatches(bound=with_args("dmcf_frs_build", args))
    assert len(bad) == 1 and bad[0].startswith("dmcf_frs_build: parameter 1 (n_points)"), bad
    f = list(fields["dmcf_cconv_args"])
    k = [n for n, _ in f].index("n_out")
    f[k] = ("n_out", ctypes.c_int32)
    bad = mismatches(fields={**fields, "dmcf_cconv_args": f})
    assert len(bad) == 1 and bad[0].startswith("struct dmcf_cconv_args.n_out"), bad
    # one parameter dropped
    args = list(bound["dmcf_frs_write"][1])
    del args[4]
    bad = mismatches(bound=with_args("dmcf_frs_write", args))
    assert len(bad) == 1 and bad[0].startswith("dmcf_frs_write: 11 argtypes, the header has 12"), bad
    # two struct fields swapped: of the same type, and of different types
    for a, b in (("extent", "window_fac"), ("n_pairs", "neighbors_row_count")):
        f = list(fields["dmcf_cconv_args"])
        i, j = [n for n, _ in f].index(a), [n for n, _ in f].index(b)
        f[i], f[j] = f[j], f[i]
        bad = mismatches(fields={**fields, "dmcf_cconv_args": f})
        assert len(bad) == 1 and bad[0].startswith("struct dmcf_cconv_args: fields"), bad
    # one array length changed
    f = list(fields["dmcf_lattice_conv_args"])
    k = [n for n, _ in f].index("base_dims")
    f[k] = ("base_dims", ctypes.c_int32 * 4)
    bad = mismatches(fields={**fields, "dmcf_lattice_conv_args": f})
    assert len(bad) == 1 and bad[0].startswith("struct dmcf_lattice_conv_args.base_dims"), bad
    # a pointer to the wrong struct mirror, a missing row, a return type
    args = list(bound["dmcf_cconv_forward"][1])
    args[0] = ctypes.POINTER(mirrors["dmcf_cconv_scatter_args"])
    bad = mismatches(bound=with_args("dmcf_cconv_forward", args))
    assert len(bad) == 1 and bad[0].startswith("dmcf_cconv_forward: parameter 0 (args)"), bad
    bad = mismatches(bound={n: p for n, p in bound.items() if n != "dmcf_emd"})
    assert bad == ["dmcf_emd: no PROTOTYPES row"]
    bad = mismatches(bound={**bound, "dmcf_frs_workspace_bytes": (ctypes.c_int, bound["dmcf_frs_workspace_bytes"][1])})
    assert len(bad) == 1 and bad[0].startswith("dmcf_frs_workspace_bytes: return"), bad


def test_constants_match_header():
    """The Python mirrors of the header's #defines and enums."""
    from dmcf_amd import _lib, ops
    c = _header_constants()
    assert (ops.FRS_IGNORE_QUERY_POINT, ops.FRS_OPEN3D_CORNER_VOXELS, ops.FRS_OPEN3D_VOXEL_WALK, ops.FRS_METRIC_LINF) == (
        c["DMCF_FRS_IGNORE_QUERY_POINT"], c["DMCF_FRS_OPEN3D_CORNER_VOXELS"], c["DMCF_FRS_OPEN3D_VOXEL_WALK"],
        c["DMCF_FRS_METRIC_LINF"])
    assert _lib.SPLAT_FARTHEST == c["DMCF_SPLAT_FARTHEST"] and _lib.SPLAT_MAX_LAYERS == c["DMCF_SPLAT_MAX_LAYERS"]
    assert ops.HIST_TILE_ROWS == c["DMCF_HIST_TILE_ROWS"]
    for name in ("FLAG_ALIGN_CORNERS", "FLAG_NORMALIZE", "FLAG_SYMMETRIC", "FLAG_ACCUMULATE", "FLAG_SKIP_SELF", "FLAG_FILTER_PACKED",
                 "ND_RELU", "ND_W_TRANSPOSED", "SPARSE_NEGATE", "SPARSE_W_TRANSPOSED", "SPARSE_ACCUMULATE"):
        assert getattr(ops, name) == c["DMCF_" + name]
    # the enums: every member has its key (None is DMCF_WINDOW_NONE; "nearest_neighbor" is DMCF_INTERP_NEAREST), no key is left over
    for table, prefix in ((ops.WINDOWS, "DMCF_WINDOW_"), (ops.MAPPINGS, "DMCF_MAP_"), (ops.INTERPOLATIONS, "DMCF_INTERP_")):
        members = {n[len(prefix):]: v for n, v in c.items() if n.startswith(prefix)}
        assert len(members) == len(table) >= 3
        for key, value in table.items():
            key = "NONE" if key is None else key.upper()
            match = [key] if key in members else [n for n in members if key.startswith(n + "_")]
            assert len(match) == 1 and members[match[0]] == value, (prefix, key)


def test_product_does_not_import_oracle():
    # the oracle is test infrastructure; nothing under dmcf_amd/ may reference it
    for dirpath, _, files in os.walk(os.path.join(ROOT, "dmcf_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "libdmcf_oracle" not in src, f


def test_ops_refuse_cpu_tensors(hip_lib):
    import torch
    from dmcf_amd import ops, _lib
    with pytest.raises(_lib.DmcfError):
        ops.fixed_radius_search(torch.zeros(4, 3), torch.zeros(4, 3), 0.5)


def test_block_diagonal_tile_mask():
    """filter_tile_mask of include/dmcf_hip.h: bit 4 * (c / 4) + o / 16 for the channels / outputs of every non-zero block."""
    from dmcf_amd import ops
    # conv200_2 (4 -> 32) + conv300_2 (8 -> 32): quad 0 feeds column tiles 0, 1; quads 1, 2 feed tiles 2, 3
    assert ops.block_diagonal_tile_mask([(0, 4, 0, 32), (4, 12, 32, 64)]) == 0b1100_1100_0011
    # blocks that straddle a quad / a tile set both
    assert ops.block_diagonal_tile_mask([(0, 6, 0, 8), (6, 8, 8, 24)]) == 0b0011_0001
    assert ops.block_diagonal_tile_mask([(0, 40, 0, 16)]) == 0 and ops.block_diagonal_tile_mask([(0, 4, 0, 80)]) == 0


def test_generated_splat_sources_are_current(tmp_path):
    """The .inc files of dmcf_amd/csrc that the splat kernels include are generated (tools/gen_*_splat.py, each with a
    PRODUCT_FILES list and write_product(outdir)) and committed: the committed text must be what the generators write."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc, tools = os.path.join(root, "dmcf_amd", "csrc"), os.path.join(root, "tools")
    names = sorted(f[:-3] for f in os.listdir(tools) if f.startswith("gen_") and f.endswith("_splat.py"))
    assert {"gen_cls_splat", "gen_z3_splat", "gen_pair_splat"} <= set(names)
    for name in names:
        spec = importlib.util.spec_from_file_location(name, os.path.join(tools, name + ".py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        gen.write_product(str(tmp_path))
        for n in gen.PRODUCT_FILES:
            assert open(os.path.join(str(tmp_path), n)).read() == open(os.path.join(csrc, n)).read(), n
