"""Reader and writer for TensorFlow 2 checkpoints (tensor-bundle format) without TensorFlow, and the mapping of a
DMCF checkpoint onto the model classes of this package.  The writer (:func:`write_bundle`, :func:`save_train_checkpoint`,
:class:`CheckpointManager`) produces the layout the reader parses, with the training loop's Adam state.

The reference saves ``tf.train.Checkpoint(step, optimizer, model)`` (pipelines/base_pipeline.py:155-169) and
restores with ``expect_partial`` (:171-187).  Format: ``ckpt.index`` is a leveldb-style
SSTable (prefix-compressed blocks + restart array, 48-byte footer with magic 0xdb4775248b80fb57) whose
values are ``BundleEntryProto`` messages {1: dtype, 2: shape, 3: shard, 4: offset, 5: size}; tensor bytes are
raw little-endian row-major in ``ckpt.data-00000-of-00001``.

Object-graph keys are attribute paths: ``model/_all_convs/<i>/1/{kernel,bias}`` (i = creation order of
PBFNet.get_cconv, models/pbf_model.py:223), ``model/denses/<l>/<s>/<k>/<i>/{kernel,bias}``,
``model/{fluid,obs}_dense/{kernel,bias}``, each followed by ``/.ATTRIBUTES/VARIABLE_VALUE``.
"""
import os
import re

import numpy as np

_MAGIC = 0xDB4775248B80FB57
_DTYPES = {1: np.float32, 2: np.float64, 3: np.int32, 9: np.int64, 10: np.bool_}


def _varint(buf, pos):
    result, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        result |= (b & 0x7F) << shift
        if not b & 0x80:
            return result, pos
        shift += 7


def _parse_block(buf, offset, size):
    """-> list of (key bytes, value bytes) of one SSTable block."""
    block = buf[offset:offset + size]
    num_restarts = int.from_bytes(block[-4:], "little")
    end = len(block) - 4 - 4 * num_restarts
    pos, key, out = 0, b"", []
    while pos < end:
        shared, pos = _varint(block, pos)
        non_shared, pos = _varint(block, pos)
        vlen, pos = _varint(block, pos)
        key = key[:shared] + bytes(block[pos:pos + non_shared])
        pos += non_shared
        out.append((key, bytes(block[pos:pos + vlen])))
        pos += vlen
    return out


def _parse_proto(buf):
    """Minimal protobuf wire parser -> {field: [values]} (varint, 64-bit, length-delimited, 32-bit)."""
    pos, out = 0, {}
    while pos < len(buf):
        tag, pos = _varint(buf, pos)
        field, wire = tag >> 3, tag & 7
        if wire == 0:
            val, pos = _varint(buf, pos)
        elif wire == 1:
            val = buf[pos:pos + 8]
            pos += 8
        elif wire == 2:
            n, pos = _varint(buf, pos)
            val = buf[pos:pos + n]
            pos += n
        elif wire == 5:
            val = buf[pos:pos + 4]
            pos += 4
        else:
            raise ValueError(f"unsupported wire type {wire}")
        out.setdefault(field, []).append(val)
    return out


def read_index(index_path):
    """-> {key: dict(dtype, shape, shard, offset, size)} for every tensor entry of ``ckpt.index``."""
    buf = open(index_path, "rb").read()
    footer = buf[-48:]
    if int.from_bytes(footer[-8:], "little") != _MAGIC:
        raise ValueError(f"{index_path}: not a tensor-bundle index (bad magic)")
    pos = 0
    _, pos = _varint(footer, pos)  # metaindex handle
    _, pos = _varint(footer, pos)
    idx_off, pos = _varint(footer, pos)
    idx_size, pos = _varint(footer, pos)
    entries = {}
    for _, handle in _parse_block(buf, idx_off, idx_size):
        off, p = _varint(handle, 0)
        size, p = _varint(handle, p)
        if buf[off + size] != 0:
            raise NotImplementedError("compressed SSTable blocks")
        for key, value in _parse_block(buf, off, size):
            if key == b"":
                continue  # bundle header
            msg = _parse_proto(value)
            shape = []
            if 2 in msg:
                for dim in _parse_proto(msg[2][0]).get(2, []):
                    shape.append(_parse_proto(dim).get(1, [0])[0])
            crc = msg.get(6, [None])[0]
            entries[key.decode()] = dict(dtype=msg.get(1, [0])[0], shape=tuple(shape), shard=msg.get(3, [0])[0],
                                         offset=msg.get(4, [0])[0], size=msg.get(5, [0])[0],
                                         crc32c=int.from_bytes(crc, "little") if crc is not None else None)
    return entries


def load_checkpoint(prefix, include_optimizer=False):
    """``prefix`` = path without ``.index`` / ``.data-...`` -> {variable path: numpy array}.
    Keys have the ``/.ATTRIBUTES/VARIABLE_VALUE`` suffix stripped; Adam slots are skipped by default."""
    entries = read_index(prefix + ".index")
    shards = {}
    out = {}
    for key, e in entries.items():
        if not key.endswith("/.ATTRIBUTES/VARIABLE_VALUE"):
            continue
        if not include_optimizer and ".OPTIMIZER_SLOT" in key:
            continue
        if e["dtype"] not in _DTYPES:
            continue
        if e["shard"] not in shards:
            cands = [f for f in os.listdir(os.path.dirname(prefix) or ".")
                     if f.startswith(os.path.basename(prefix) + ".data-%05d-of-" % e["shard"])]
            if not cands:
                raise FileNotFoundError(f"data shard {e['shard']} of {prefix} is missing")
            shards[e["shard"]] = np.memmap(os.path.join(os.path.dirname(prefix) or ".", cands[0]), dtype=np.uint8,
                                           mode="r")
        raw = shards[e["shard"]][e["offset"]:e["offset"] + e["size"]]
        arr = np.frombuffer(bytes(raw), dtype=_DTYPES[e["dtype"]]).reshape(e["shape"])
        out[key[:-len("/.ATTRIBUTES/VARIABLE_VALUE")]] = arr
    return out


def _assign(module, attr, value, device):
    import torch
    t = torch.from_numpy(np.array(value, copy=True)).to(device)
    setattr(module, attr, torch.nn.Parameter(t, requires_grad=False))
    if hasattr(module, "invalidate_packed"):
        module.invalidate_packed()


def model_weight_items(model):
    """-> list of ([candidate checkpoint key prefixes], module) for every weight-bearing layer of a
    PBFNet-family model.  TensorFlow names a variable by the shortest attribute path to it, so a conv that
    is also a direct attribute is stored under that name (``model/fluid_convs``, ``model/obs_convs``,
    ``model/sym_convs/<i>``, ``model/adv_convs/<i>``) and all others under ``model/_all_convs/<i>/1``
    (observed in checkpoints/*/ckpt.index).  A model with a ``checkpoint_items()`` method (PointNet) lists its own."""
    own = getattr(model, "checkpoint_items", None)
    if own is not None:
        return own()
    alias = {id(model.fluid_convs): "model/fluid_convs", id(model.obs_convs): "model/obs_convs"}
    for i, conv in enumerate(getattr(model, "sym_convs", [])):
        alias[id(conv)] = f"model/sym_convs/{i}"
    for i, conv in enumerate(getattr(model, "adv_convs", []) or []):
        alias[id(conv)] = f"model/adv_convs/{i}"
    items = []
    for i, (_, conv) in enumerate(model._all_convs):
        cands = [f"model/_all_convs/{i}/1"]
        if id(conv) in alias:
            cands.insert(0, alias[id(conv)])
        items.append((cands, conv))
    items.append((["model/fluid_dense"], model.fluid_dense))
    items.append((["model/obs_dense"], model.obs_dense))
    if getattr(model, "equivar", False):  # models/pbf_model.py:183-189
        items.append((["model/scale_dens"], model.scale_dens))
        items.append((["model/rot_dens"], model.rot_dens))
    for i, dense in enumerate(getattr(model, "adv_dense", []) or []):
        items.append(([f"model/adv_dense/{i}"], dense))
    denses = getattr(model, "denses", [])
    if denses and isinstance(denses[0], list):  # HRNet / SymNet: denses[layer][scale][k][inp]
        for a, la in enumerate(denses):
            for b, lb in enumerate(la):
                for c, lc in enumerate(lb):
                    for d, dense in enumerate(lc):
                        items.append(([f"model/denses/{a}/{b}/{c}/{d}"], dense))
    else:  # CConv: flat list
        for a, dense in enumerate(denses):
            items.append(([f"model/denses/{a}"], dense))
    return items


def load_into_model(model, weights, device="cuda", strict=True):
    """Assign ``weights`` ({key: array} from :func:`load_checkpoint` or an ``.npz``) to ``model``.
    Layers the checkpoint has no entry for stay lazily initialised (``expect_partial`` semantics,
    pipelines/base_pipeline.py:172-173; e.g. the never-called cross-scale Dense layers); with ``strict``
    every conv kernel must be present.  Returns the number of layers loaded."""
    loaded = 0
    for cands, module in model_weight_items(model):
        prefix = next((c for c in cands if c + "/kernel" in weights), None)
        if prefix is None:
            if strict and hasattr(module, "fixed_radius_search"):
                raise KeyError(f"{cands}: kernel missing from the checkpoint")
            continue
        k = weights[prefix + "/kernel"]
        if hasattr(module, "in_channels"):  # ContinuousConv
            module.in_channels = int(k.shape[-2])
        _assign(module, "kernel", k, device)
        loaded += 1
        b = weights.get(prefix + "/bias")
        if b is not None and getattr(module, "use_bias", True):
            _assign(module, "bias", b, device)
    return loaded


def checkpoint_epoch(path, save_ckpt_freq=1):
    """Epoch recovered from the name of a checkpoint manager's newest checkpoint, like the reference
    (pipelines/base_pipeline.py:182-185): ``(n - 1) * save_ckpt_freq + 1`` for ``ckpt-<n>``."""
    nums = re.findall(r"\d+", os.path.basename(path))
    return (int(nums[-1]) - 1) * int(save_ckpt_freq) + 1 if nums else 0


# ---- writer ------------------------------------------------------------------------------------------------------------
# The same tensor-bundle layout TensorFlow's BundleWriter produces (tensorflow/core/util/tensor_bundle): tensor bytes in the
# order they are added, one data shard; an SSTable index (leveldb table format, uncompressed, one data block up to 256 KiB,
# a restart point every 16 keys, prefix-compressed keys, block trailers with a masked crc32c, an empty metaindex block,
# an index block whose single key is the shortest successor of the last key, the 48-byte footer with the magic).

_DTYPE_CODES = {np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.int32): 3, np.dtype(np.int64): 9,
                np.dtype(np.bool_): 10}
DT_STRING = 7
_BLOCK_SIZE = 262144  # tensorflow/core/lib/io/table_options.h
_RESTART_INTERVAL = 16
_SLOT = "/.OPTIMIZER_SLOT/optimizer/"
_VALUE = "/.ATTRIBUTES/VARIABLE_VALUE"
OBJECT_GRAPH_KEY = "_CHECKPOINTABLE_OBJECT_GRAPH"


def _crc_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        table.append(c)
    return table


_CRC_TABLE = _crc_table()


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli) of ``data``, continuing from ``crc`` (crc32c::Extend)."""
    t = _CRC_TABLE
    c = crc ^ 0xFFFFFFFF
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def mask_crc(crc):
    """crc32c::Mask: the form leveldb / TensorFlow store."""
    return ((((crc >> 15) | (crc << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def _put_varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _field_varint(field, value):
    return _put_varint(field << 3) + _put_varint(value) if value else b""


def _field_bytes(field, value):
    return _put_varint((field << 3) | 2) + _put_varint(len(value)) + value


def _entry_proto(e):
    """BundleEntryProto {1 dtype, 2 shape {2 dim {1 size}}, 3 shard_id, 4 offset, 5 size, 6 crc32c (fixed32)} in field order,
    proto3: zero scalars omitted, the shape always present."""
    shape = b"".join(_field_bytes(2, _field_varint(1, int(d))) for d in e["shape"])
    return (_field_varint(1, e["dtype"]) + _field_bytes(2, shape) + _field_varint(3, e.get("shard", 0))
            + _field_varint(4, e["offset"]) + _field_varint(5, e["size"])
            + _put_varint((6 << 3) | 5) + int(e["crc32c"]).to_bytes(4, "little"))


def _bundle_header():
    """BundleHeaderProto {num_shards: 1, endianness: LITTLE, version {producer: 1}}."""
    return _field_varint(1, 1) + _field_bytes(3, _field_varint(1, 1))


class _BlockBuilder:
    def __init__(self, restart_interval):
        self.buf, self.restarts, self.counter, self.last = bytearray(), [0], 0, b""
        self.interval = restart_interval

    def add(self, key, value):
        shared = 0
        if self.counter < self.interval:
            n = min(len(self.last), len(key))
            while shared < n and self.last[shared] == key[shared]:
                shared += 1
        else:
            self.restarts.append(len(self.buf))
            self.counter = 0
        self.buf += _put_varint(shared) + _put_varint(len(key) - shared) + _put_varint(len(value))
        self.buf += key[shared:] + value
        self.last, self.counter = key, self.counter + 1

    def size_estimate(self):
        return len(self.buf) + 4 * len(self.restarts) + 4

    def finish(self):
        return bytes(self.buf) + b"".join(r.to_bytes(4, "little") for r in self.restarts) + len(self.restarts).to_bytes(4, "little")

    def empty(self):
        return not self.buf


def _short_successor(key):
    """leveldb BytewiseComparator::FindShortSuccessor."""
    for i, b in enumerate(key):
        if b != 0xFF:
            return key[:i] + bytes([b + 1])
    return key


def _short_separator(start, limit):
    """leveldb BytewiseComparator::FindShortestSeparator."""
    n = min(len(start), len(limit))
    i = 0
    while i < n and start[i] == limit[i]:
        i += 1
    if i < n:
        b = start[i]
        if b < 0xFF and b + 1 < limit[i]:
            return start[:i] + bytes([b + 1])
    return start


def encode_index(entries):
    """{key: dict(dtype, shape, shard, offset, size, crc32c)} -> the bytes of a bundle's ``.index`` file (keys sorted
    bytewise after the header entry, which has the empty key)."""
    out = bytearray()
    index = _BlockBuilder(1)  # (leveldb's index block: a restart point per key)

    def write_block(block):
        raw = block.finish()
        handle = (len(out), len(raw))
        out.extend(raw)
        out.extend(b"\x00" + mask_crc(crc32c(b"\x00", crc32c(raw))).to_bytes(4, "little"))
        return handle

    def handle_bytes(h):
        return _put_varint(h[0]) + _put_varint(h[1])

    data = _BlockBuilder(_RESTART_INTERVAL)
    pending, last = None, b""
    items = [(b"", _bundle_header())] + [(k.encode(), _entry_proto(e)) for k, e in sorted(entries.items(), key=lambda kv: kv[0].encode())]
    for key, value in items:
        if pending is not None:
            index.add(_short_separator(last, key), handle_bytes(pending))
            pending = None
        data.add(key, value)
        last = key
        if data.size_estimate() >= _BLOCK_SIZE:
            pending = write_block(data)
            data = _BlockBuilder(_RESTART_INTERVAL)
    if not data.empty():
        pending = write_block(data)
    meta = write_block(_BlockBuilder(_RESTART_INTERVAL))
    if pending is not None:
        index.add(_short_successor(last), handle_bytes(pending))
    idx = write_block(index)
    footer = bytearray(handle_bytes(meta) + handle_bytes(idx))
    footer += bytes(40 - len(footer))
    out += footer + _MAGIC.to_bytes(8, "little")
    return bytes(out)


def _string_tensor_bytes(value):
    """A scalar DT_STRING tensor as BundleWriter stores it (WriteStringTensor): varint64 length, the masked crc32c of the
    length (taken over it as a uint32 below 2^32, as a uint64 above), the bytes.  -> (stored bytes, crc32c of the entry,
    unmasked)."""
    n = len(value)
    crc = crc32c(n.to_bytes(4 if n <= 0xFFFFFFFF else 8, "little"))
    masked = mask_crc(crc)
    crc = crc32c(masked.to_bytes(4, "little"), crc)
    crc = crc32c(value, crc)
    return _put_varint(n) + masked.to_bytes(4, "little") + bytes(value), crc


def write_bundle(prefix, tensors):
    """Write ``tensors`` -- (key, value) pairs in the order their bytes go to the data file; a value is a numpy array
    (float32 / float64 / int32 / int64 / bool) or ``bytes`` (a scalar string tensor: the object graph) -- as
    ``<prefix>.index`` and ``<prefix>.data-00000-of-00001``.  Returns the index entries."""
    entries, offset = {}, 0
    os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
    with open(prefix + ".data-00000-of-00001.tmp", "wb") as f:
        for key, value in tensors:
            if isinstance(value, (bytes, bytearray)):
                raw, crc = _string_tensor_bytes(value)
                dtype, shape = DT_STRING, ()
            else:
                arr = np.asarray(value, order="C")
                if arr.dtype not in _DTYPE_CODES:
                    raise TypeError(f"{key}: dtype {arr.dtype} cannot be written")
                raw = arr.astype(arr.dtype.newbyteorder("<"), copy=False).tobytes()
                dtype, shape, crc = _DTYPE_CODES[arr.dtype], arr.shape, crc32c(raw)
            if key in entries:
                raise ValueError(f"duplicate key {key}")
            entries[key] = dict(dtype=dtype, shape=tuple(int(d) for d in shape), shard=0, offset=offset, size=len(raw),
                                crc32c=mask_crc(crc))
            f.write(raw)
            offset += len(raw)
    index = encode_index(entries)
    with open(prefix + ".index.tmp", "wb") as f:
        f.write(index)
    os.replace(prefix + ".data-00000-of-00001.tmp", prefix + ".data-00000-of-00001")
    os.replace(prefix + ".index.tmp", prefix + ".index")
    return entries


def read_bundle(prefix):
    """Every entry of a single-shard bundle in data-file order -> list of (key, value): numpy arrays, and ``bytes`` for
    scalar string tensors (the object graph)."""
    entries = read_index(prefix + ".index")
    data = open(prefix + ".data-00000-of-00001", "rb").read()
    out = []
    for key, e in sorted(entries.items(), key=lambda kv: kv[1]["offset"]):
        if e["shard"] != 0:
            raise NotImplementedError("multi-shard bundles")
        raw = data[e["offset"]:e["offset"] + e["size"]]
        if e["dtype"] == DT_STRING:
            if e["shape"] != ():
                raise NotImplementedError(f"{key}: string tensors of rank > 0")
            n, p = _varint(raw, 0)
            out.append((key, bytes(raw[p + 4:p + 4 + n])))
        elif e["dtype"] in _DTYPES:
            out.append((key, np.frombuffer(raw, dtype=_DTYPES[e["dtype"]]).reshape(e["shape"]).copy()))
        else:
            raise NotImplementedError(f"{key}: dtype {e['dtype']}")
    return out


def model_variables(model):
    """-> [(checkpoint key without the VARIABLE_VALUE suffix, module, attribute)] of every built weight of ``model``: each
    layer under the first candidate of :func:`model_weight_items` (the name TensorFlow gives it), kernel before bias."""
    out = []
    for cands, module in model_weight_items(model):
        for attr in ("kernel", "bias"):
            if getattr(module, attr, None) is not None:
                out.append((f"{cands[0]}/{attr}", module, attr))
    return out


def save_train_checkpoint(prefix, model, optimizer, save_counter, object_graph=None):
    """Write the reference's ``tf.train.Checkpoint(step, optimizer, model)`` (pipelines/base_pipeline.py:159-162) as a bundle:
    ``step`` (int32 1: the reference never advances it), ``save_counter`` (int64), ``optimizer/{iter, beta_1, beta_2, decay}``,
    every model variable and, for the variables that have them, the Adam slots ``.OPTIMIZER_SLOT/optimizer/{m, v}``.
    ``object_graph``: the ``_CHECKPOINTABLE_OBJECT_GRAPH`` bytes of the checkpoint the run started from, copied byte for byte
    (the keys here are the ones it names).  A run from scratch has none and writes none: TensorFlow's object-based restore
    then cannot read the file (its name-based form, and this package's reader, can)."""
    variables = model_variables(model)
    slots = optimizer.slots_by_param()
    tensors = [("step" + _VALUE, np.array(1, np.int32)), ("save_counter" + _VALUE, np.array(save_counter, np.int64)),
               ("optimizer/iter" + _VALUE, np.array(optimizer.iterations, np.int64)),
               ("optimizer/beta_1" + _VALUE, np.array(optimizer.beta_1, np.float32)),
               ("optimizer/beta_2" + _VALUE, np.array(optimizer.beta_2, np.float32)),
               ("optimizer/decay" + _VALUE, np.array(optimizer.decay, np.float32))]
    host = lambda t: t.detach().cpu().numpy().astype(np.float32, copy=False)  # noqa: E731
    tensors += [(key + _VALUE, host(getattr(mod, attr))) for key, mod, attr in variables]
    for k in ("m", "v"):
        for key, mod, attr in variables:
            s = slots.get(id(getattr(mod, attr)))
            if s is not None:
                tensors.append((key + _SLOT + k + _VALUE, host(s[k])))
    if object_graph is not None:
        tensors.append((OBJECT_GRAPH_KEY, bytes(object_graph)))
    return write_bundle(prefix, tensors)


def read_train_state(prefix):
    """The training state of a bundle: ({variable key: array}, {variable key: (m, v)}, {'iter', 'beta_1', 'beta_2', 'decay',
    'save_counter'}, object graph bytes or None)."""
    weights, slots, opt, graph = {}, {}, {}, None
    for key, value in read_bundle(prefix):
        if key == OBJECT_GRAPH_KEY:
            graph = value
            continue
        if not key.endswith(_VALUE):
            continue
        key = key[:-len(_VALUE)]
        if _SLOT in key:
            var, k = key.split(_SLOT)
            slots.setdefault(var, {})[k] = value
        elif key.startswith("optimizer/"):
            opt[key[len("optimizer/"):]] = value[()]
        elif key == "save_counter":
            opt["save_counter"] = int(value)
        elif key.startswith("model/"):
            weights[key] = value
    return weights, slots, opt, graph


class CheckpointManager:
    """tf.train.CheckpointManager(ckpt, <logs_dir>/checkpoint, max_to_keep=100) (pipelines/base_pipeline.py:164-166):
    ``save()`` writes ``ckpt-<save_counter>`` and the ``checkpoint`` state file and drops the oldest checkpoints beyond
    ``max_to_keep``; ``latest_checkpoint`` is the newest prefix listed there (None without one)."""

    def __init__(self, directory, max_to_keep=100):
        self.directory, self.max_to_keep = directory, int(max_to_keep)
        os.makedirs(directory, exist_ok=True)
        self.paths, self.timestamps = self._read_state()

    def _read_state(self):
        path = os.path.join(self.directory, "checkpoint")
        paths, stamps = [], []
        if os.path.exists(path):
            for line in open(path):
                m = re.match(r'\s*all_model_checkpoint_paths:\s*"(.*)"', line)
                if m:
                    paths.append(m.group(1))
                m = re.match(r"\s*all_model_checkpoint_timestamps:\s*([0-9.eE+-]+)", line)
                if m:
                    stamps.append(float(m.group(1)))
        paths = [p for p in paths if os.path.exists(self._abs(p) + ".index")]
        return paths, (stamps if len(stamps) == len(paths) else [0.0] * len(paths))

    def _abs(self, p):
        return p if os.path.isabs(p) else os.path.join(self.directory, p)

    @property
    def latest_checkpoint(self):
        return self._abs(self.paths[-1]) if self.paths else None

    def save(self, model, optimizer, save_counter, object_graph=None):
        import time
        name = f"ckpt-{int(save_counter)}"
        save_train_checkpoint(os.path.join(self.directory, name), model, optimizer, save_counter, object_graph)
        if name in self.paths:
            i = self.paths.index(name)
            del self.paths[i], self.timestamps[i]
        self.paths.append(name)
        self.timestamps.append(time.time())
        while len(self.paths) > self.max_to_keep:
            old = self.paths.pop(0)
            self.timestamps.pop(0)
            for suffix in (".index", ".data-00000-of-00001"):
                if os.path.exists(self._abs(old) + suffix):
                    os.remove(self._abs(old) + suffix)
        lines = [f'model_checkpoint_path: "{self.paths[-1]}"']
        lines += [f'all_model_checkpoint_paths: "{p}"' for p in self.paths]
        lines += [f"all_model_checkpoint_timestamps: {t:.6f}" for t in self.timestamps]
        lines.append(f"last_preserved_timestamp: {self.timestamps[0]:.6f}")
        with open(os.path.join(self.directory, "checkpoint.tmp"), "w") as f:
            f.write("\n".join(lines) + "\n")
        os.replace(os.path.join(self.directory, "checkpoint.tmp"), os.path.join(self.directory, "checkpoint"))
        return os.path.join(self.directory, name)
