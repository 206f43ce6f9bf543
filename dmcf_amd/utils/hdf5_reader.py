"""Reading result files back without h5py: the HDF5 subset ``hdf5_writer.write_hdf5`` writes (and ``write_results`` through it),
plus the ``.npz`` stand-in of ``write_results_npz``.  ``utils/draw_sim2d.py:170-174`` of the reference reads these files through
h5py; :func:`read_results` does the same when h5py is importable, as ``write_results`` does.

What is understood (HDF5 File Format Specification): a version-0 superblock with 8-byte offsets and lengths; version-1 object
headers (continuation messages followed); "old style" groups (symbol table message, version-1 group B-tree of any depth, symbol
table nodes, local heap); datasets with a dataspace message (version 1 or 2), a datatype message of class 0 (little-endian
two's-complement integers), 1 (little-endian IEEE binary32 / binary64: implied leading bit, sign in the top bit) or 3
(fixed-length, null-terminated or null-padded ASCII / UTF-8 strings), a version-3 data layout
message (contiguous or compact) and version-1 attribute messages.  Anything else -- another superblock or object header
version, new-style groups, chunked or external storage, filters, shared messages, other datatypes -- raises ``ValueError``
naming it, rather than being misread.
"""
import os
import struct

import numpy as np

UNDEF = 0xFFFFFFFFFFFFFFFF
SIGNATURE = b"\x89HDF\r\n\x1a\n"
# messages that carry nothing the data depends on: NIL, fill value (old / new: the writer allocates every non-empty dataset),
# comment, modification time (old / new)
_IGNORED = {0x0000: "NIL", 0x0004: "fill value (old)", 0x0005: "fill value", 0x000D: "comment", 0x000E: "modification time (old)",
            0x0012: "modification time"}


class _File:
    def __init__(self, f, size):
        self.f, self.size = f, size

    def read(self, at, n, what):
        if at == UNDEF or at < 0 or at + n > self.size:
            raise ValueError(f"HDF5: {what} at {at:#x} (+{n}) lies outside the file ({self.size} bytes): truncated or not supported")
        self.f.seek(at)
        return self.f.read(n)


def _dtype(msg):
    """numpy dtype (or ('S', n)) of a datatype message."""
    if len(msg) < 8:
        raise ValueError("HDF5: short datatype message")
    cls, version = msg[0] & 0x0F, msg[0] >> 4
    bits = msg[1] | (msg[2] << 8) | (msg[3] << 16)
    size = struct.unpack_from("<I", msg, 4)[0]
    if version != 1:
        raise ValueError(f"HDF5: datatype message version {version} is not supported")
    if cls == 0:  # fixed point
        if bits & 0x1:
            raise ValueError("HDF5: big-endian integer datatype is not supported")
        offset, precision = struct.unpack_from("<HH", msg, 8)
        if size not in (1, 2, 4, 8) or offset != 0 or precision != 8 * size:
            raise ValueError(f"HDF5: integer datatype of {size} bytes, bit offset {offset}, precision {precision} is not supported")
        return np.dtype(("<i%d" if bits & 0x8 else "<u%d") % size)
    if cls == 1:  # floating point
        if bits & 0x41:
            raise ValueError("HDF5: big-endian or VAX floating-point datatype is not supported")
        if bits & 0x0E:
            raise ValueError("HDF5: floating-point datatype with padding bits set is not supported")
        if (bits >> 4) & 0x3 != 2:
            raise ValueError(f"HDF5: floating-point mantissa normalisation {(bits >> 4) & 0x3} is not supported (2, an implied "
                             "leading bit, only)")
        offset, precision, exp_loc, exp_size, man_loc, man_size, bias = struct.unpack_from("<HHBBBBI", msg, 8)
        if (bits >> 8) & 0xFF != precision - 1:
            raise ValueError(f"HDF5: floating-point sign bit at {(bits >> 8) & 0xFF} is not supported (the top bit only)")
        ieee = {4: (32, 23, 8, 23, 0, 127), 8: (64, 52, 11, 52, 0, 1023)}
        if ieee.get(size) != (precision, exp_loc, exp_size, man_size, man_loc, bias) or offset != 0:
            raise ValueError(f"HDF5: floating-point datatype of {size} bytes is not IEEE binary32 / binary64 (not supported)")
        return np.dtype("<f%d" % size)
    if cls == 3:  # fixed-length string: null terminated or null padded (trailing NULs dropped), ASCII or UTF-8
        if bits & 0x0F not in (0, 1):
            raise ValueError(f"HDF5: string padding type {bits & 0x0F} is not supported (null terminated or null padded only)")
        if (bits >> 4) & 0x0F not in (0, 1):
            raise ValueError(f"HDF5: string character set {(bits >> 4) & 0x0F} is not supported (ASCII or UTF-8 only)")
        return ("S", size)
    names = {2: "time", 4: "bitfield", 5: "opaque", 6: "compound", 7: "reference", 8: "enumeration", 9: "variable-length",
             10: "array"}
    raise ValueError(f"HDF5: datatype class {cls} ({names.get(cls, 'unknown')}) is not supported")


def _dataspace(msg):
    version, rank, flags = msg[0], msg[1], msg[2]
    if version == 1:
        at = 8
    elif version == 2:
        if msg[3] == 2:  # null dataspace
            return None
        at = 4
    else:
        raise ValueError(f"HDF5: dataspace message version {version} is not supported")
    return tuple(struct.unpack_from("<%dQ" % rank, msg, at)) if rank else ()


def _values(raw, dtype, shape):
    if isinstance(dtype, tuple):  # strings: scalars come back as str, arrays as bytes arrays
        n = dtype[1]
        count = int(np.prod(shape)) if shape else 1
        if len(raw) < n * count:
            raise ValueError("HDF5: string data shorter than its dataspace")
        arr = np.frombuffer(raw[:n * count], dtype="S%d" % n).reshape(shape)
        return arr[()].split(b"\0", 1)[0].decode("utf-8") if shape == () else arr
    count = int(np.prod(shape)) if shape else 1
    if len(raw) < dtype.itemsize * count:
        raise ValueError("HDF5: data shorter than its dataspace")
    return np.frombuffer(raw[:dtype.itemsize * count], dtype=dtype).reshape(shape).copy()


def _attribute(msg):
    version = msg[0]
    if version != 1:
        raise ValueError(f"HDF5: attribute message version {version} is not supported")
    name_size, dt_size, ds_size = struct.unpack_from("<HHH", msg, 2)
    pad = lambda n: n + (-n % 8)  # noqa: E731
    at = 8
    name = msg[at:at + name_size].split(b"\0", 1)[0].decode("ascii")
    at += pad(name_size)
    dtype = _dtype(msg[at:at + dt_size])
    at += pad(dt_size)
    shape = _dataspace(msg[at:at + ds_size])
    at += pad(ds_size)
    if shape is None:
        raise ValueError(f"HDF5: attribute {name!r} has a null dataspace (not supported)")
    return name, _values(msg[at:], dtype, shape)


def _messages(F, at):
    """[(type, flags, data)] of the version-1 object header at ``at``, continuation blocks followed."""
    head = F.read(at, 16, "object header")
    version, _, count, _, size = struct.unpack("<BBHII", head[:12])
    if version != 1:
        raise ValueError(f"HDF5: object header version {version} at {at:#x} is not supported (version 1 only)")
    blocks, out = [(at + 16, size)], []
    while blocks and len(out) < count:
        start, length = blocks.pop(0)
        raw = F.read(start, length, "object header messages")
        pos = 0
        while pos + 8 <= length and len(out) < count:
            mtype, msize, mflags = struct.unpack_from("<HHB", raw, pos)
            data = raw[pos + 8:pos + 8 + msize]
            pos += 8 + msize
            if mflags & 0x02:
                raise ValueError(f"HDF5: shared message (type {mtype:#06x}) is not supported")
            if mtype == 0x0010:  # continuation
                blocks.append(struct.unpack_from("<QQ", data))
            out.append((mtype, mflags, data))
    if len(out) < count:
        raise ValueError(f"HDF5: object header at {at:#x} holds fewer messages than it declares")
    return out


def _heap_name(F, heap, off):
    raw = F.read(heap[1] + off, min(256, heap[0] - off), "local heap name") if off < heap[0] else b""
    if b"\0" not in raw:
        raise ValueError("HDF5: link name outside the local heap")
    return raw.split(b"\0", 1)[0].decode("utf-8")


def _group_members(F, btree, heap_at):
    """{name: object header address} of an old-style group (B-tree version 1, type 0, any depth)."""
    h = F.read(heap_at, 32, "local heap")
    if h[:4] != b"HEAP" or h[4] != 0:
        raise ValueError(f"HDF5: no version-0 local heap at {heap_at:#x}")
    heap = struct.unpack_from("<QQQ", h, 8)
    heap = (heap[0], heap[2])  # (data segment size, data segment address)
    members, todo, seen = {}, [btree], set()
    while todo:
        node = todo.pop()
        if node in seen:
            raise ValueError("HDF5: cycle in a group B-tree")
        seen.add(node)
        t = F.read(node, 24, "group B-tree node")
        if t[:4] != b"TREE" or t[4] != 0:
            raise ValueError(f"HDF5: no version-1 group B-tree node at {node:#x}")
        level, used = t[5], struct.unpack_from("<H", t, 6)[0]
        body = F.read(node + 24, 16 * used + 8, "group B-tree keys")
        children = [struct.unpack_from("<Q", body, 8 + 16 * i)[0] for i in range(used)]
        if level > 0:
            todo.extend(children)
            continue
        for snod in children:
            s = F.read(snod, 8, "symbol table node")
            if s[:4] != b"SNOD" or s[4] != 1:
                raise ValueError(f"HDF5: no version-1 symbol table node at {snod:#x}")
            n = struct.unpack_from("<H", s, 6)[0]
            raw = F.read(snod + 8, 40 * n, "symbol table entries")
            for i in range(n):
                name_off, header = struct.unpack_from("<QQ", raw, 40 * i)
                members[_heap_name(F, heap, name_off)] = header
    return members


def _object(F, at, depth=0):
    """A group -> {name: member}; a dataset -> (array, {attribute: value})."""
    if depth > 32:
        raise ValueError("HDF5: groups nested too deeply")
    msgs = _messages(F, at)
    types = {m[0] for m in msgs}
    for mtype, _, _ in msgs:
        if mtype in (0x0002, 0x0006, 0x000A):
            raise ValueError(f"HDF5: new-style group (link message {mtype:#06x}) is not supported")
        if mtype == 0x0007:
            raise ValueError("HDF5: external data files are not supported")
        if mtype == 0x000B:
            raise ValueError("HDF5: filter pipeline (compressed or filtered data) is not supported")
        if mtype not in _IGNORED and mtype not in (0x0001, 0x0003, 0x0008, 0x000C, 0x0010, 0x0011):
            raise ValueError(f"HDF5: object header message type {mtype:#06x} is not supported")
    if 0x0011 in types:
        btree, heap = struct.unpack_from("<QQ", next(m[2] for m in msgs if m[0] == 0x0011))
        return {name: _object(F, h, depth + 1) for name, h in _group_members(F, btree, heap).items()}
    if not {0x0001, 0x0003, 0x0008} <= types:
        raise ValueError(f"HDF5: object at {at:#x} is neither an old-style group nor a dataset")
    shape = _dataspace(next(m[2] for m in msgs if m[0] == 0x0001))
    dtype = _dtype(next(m[2] for m in msgs if m[0] == 0x0003))
    layout = next(m[2] for m in msgs if m[0] == 0x0008)
    if layout[0] != 3:
        raise ValueError(f"HDF5: data layout message version {layout[0]} is not supported (version 3 only)")
    if shape is None:
        raise ValueError("HDF5: dataset with a null dataspace is not supported")
    itemsize = dtype[1] if isinstance(dtype, tuple) else dtype.itemsize
    nbytes = itemsize * (int(np.prod(shape)) if shape else 1)
    if layout[1] == 0:  # compact
        size = struct.unpack_from("<H", layout, 2)[0]
        raw = layout[4:4 + size]
    elif layout[1] == 1:  # contiguous
        addr, size = struct.unpack_from("<QQ", layout, 2)
        if size < nbytes:
            raise ValueError("HDF5: contiguous storage smaller than the dataspace")
        raw = b"" if nbytes == 0 else F.read(addr, nbytes, "dataset data")
    else:
        raise ValueError(f"HDF5: data layout class {layout[1]} ({'chunked' if layout[1] == 2 else 'virtual'}) is not supported")
    attrs = dict(_attribute(m[2]) for m in msgs if m[0] == 0x000C)
    return _values(raw, dtype, shape), attrs


def read_hdf5(path):
    """The file's root group as {name: member}: a group is a dict of its members, a dataset an (array, {attribute: value})
    pair (string attributes as str).  Reads what :func:`dmcf_amd.utils.hdf5_writer.write_hdf5` writes; refuses with a
    ``ValueError`` whatever lies outside the subset named in the module docstring."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        F = _File(f, size)
        sb = F.read(0, 96, "superblock")
        if sb[:8] != SIGNATURE:
            raise ValueError(f"{path}: not an HDF5 file (no signature at offset 0; user blocks are not supported)")
        if sb[8] != 0:
            raise ValueError(f"HDF5: superblock version {sb[8]} is not supported (version 0 only)")
        if sb[13] != 8 or sb[14] != 8:
            raise ValueError(f"HDF5: {sb[13]}-byte offsets / {sb[14]}-byte lengths are not supported (8 only)")
        base = struct.unpack_from("<Q", sb, 24)[0]
        if base != 0:
            raise ValueError("HDF5: a base address other than 0 is not supported")
        root = struct.unpack_from("<Q", sb, 56 + 8)[0]
        out = _object(F, root)
        if not isinstance(out, dict):
            raise ValueError("HDF5: the root object is not a group")
        return out


def read_results(path):
    """A result file of ``write_results`` / ``write_results_npz`` as {group: {dataset: (array, {attribute: value})}}.  ``.npz``:
    the stand-in's ``<group>/<dataset>`` arrays with their ``type``, ``dim`` = the shape (what write_results stores).  HDF5:
    through h5py when it is importable, otherwise :func:`read_hdf5`."""
    if str(path).endswith(".npz"):
        out = {}
        with np.load(path) as z:
            for key in z.files:
                if key.endswith(".type"):
                    continue
                group, name = key.split("/", 1)
                arr = z[key]
                attrs = {"dim": np.asarray(arr.shape, dtype=np.int64)}
                if key + ".type" in z.files:
                    attrs["type"] = str(z[key + ".type"][()])
                out.setdefault(group, {})[name] = (arr, attrs)
        return out
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None:
        with h5py.File(path, "r") as h:
            return {g: {k: (v[()], {a: (x.decode() if isinstance(x, bytes) else x) for a, x in v.attrs.items()})
                        for k, v in h[g].items()} for g in h}
    root = read_hdf5(path)
    for g, members in root.items():
        if not isinstance(members, dict) or any(isinstance(m, dict) for m in members.values()):
            raise ValueError(f"{path}: {g!r} is not a group of datasets (not a result file)")
    return root
