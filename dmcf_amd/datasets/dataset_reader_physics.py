"""Scene files and rollouts -- the inference-side part of the reference's ``datasets/dataset_reader_physics.py``
(same function / class names where they exist there):

  Dataset            :179-207  a directory of ``*.msgpack.zst`` scene files, or in-memory scenes
  read_scene / write_scene     one scene file = one zstd frame holding a msgpack list of per-frame dicts whose
                               ndarrays use the msgpack-numpy encoding {nd, type, kind, shape, data}
                               (``load_data`` of run_sample.py:200-205, cache writer :168-176)
  get_rollout        :410-456  per-scene dicts of stacked frames (pos [T,N,3], vel, grav broadcast to [T,N,3], box ...)
                               with the translate / scale / grav_eqvar input transform of :276-293
  write_results      :520-526  HDF5 result file (needs h5py, which this image lacks: raises a clear error) and an
                               .npz stand-in with the same content

  PhysicsSimDataFlow :210-357  training samples: windows of pre + window + 1 frames, augmentation, input transform
  get_dataloader     :469-517  repeat, a seeded local shuffle buffer, list batching (the training loop's loader)

zstd comes from the system ``libzstd.so.1`` through ctypes; msgpack from the ``msgpack`` package.  The column / free-fall
generators of the training side are not rebuilt (pass scene files or in-memory scenes).
"""
import ctypes
import ctypes.util
import glob
import os

import msgpack
import numpy as np

_zstd = None


def _libzstd():
    global _zstd
    if _zstd is None:
        name = ctypes.util.find_library("zstd") or "libzstd.so.1"
        z = ctypes.CDLL(name)
        z.ZSTD_getFrameContentSize.restype = ctypes.c_ulonglong
        z.ZSTD_getFrameContentSize.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        z.ZSTD_decompress.restype = ctypes.c_size_t
        z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        z.ZSTD_compressBound.restype = ctypes.c_size_t
        z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        z.ZSTD_compress.restype = ctypes.c_size_t
        z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        z.ZSTD_isError.restype = ctypes.c_uint
        z.ZSTD_isError.argtypes = [ctypes.c_size_t]
        _zstd = z
    return _zstd


def zstd_decompress(raw):
    z = _libzstd()
    n = z.ZSTD_getFrameContentSize(raw, len(raw))
    if n in (2 ** 64 - 1, 2 ** 64 - 2):  # ZSTD_CONTENTSIZE_UNKNOWN / _ERROR
        raise ValueError("not a zstd frame with a known content size")
    buf = ctypes.create_string_buffer(max(int(n), 1))
    r = z.ZSTD_decompress(buf, n, raw, len(raw))
    if z.ZSTD_isError(r):
        raise ValueError("zstd decompression failed")
    return buf.raw[:r]


def zstd_compress(data, level=19):
    z = _libzstd()
    cap = z.ZSTD_compressBound(len(data))
    buf = ctypes.create_string_buffer(cap)
    r = z.ZSTD_compress(buf, cap, data, len(data), level)
    if z.ZSTD_isError(r):
        raise ValueError("zstd compression failed")
    return buf.raw[:r]


def _decode(o):
    """msgpack-numpy object hook (keys may arrive as str or bytes)."""
    if isinstance(o, dict):
        nd = o.get("nd", o.get(b"nd"))
        if nd is not None and ("type" in o or b"type" in o):
            g = lambda k: o.get(k, o.get(k.encode()))  # noqa: E731
            dtype = g("type")
            dtype = np.dtype(dtype.decode() if isinstance(dtype, bytes) else dtype)
            if nd:
                return np.frombuffer(g("data"), dtype=dtype).reshape(g("shape")).copy()
            return np.frombuffer(g("data"), dtype=dtype)[0]
    return o


def _encode(o):
    """msgpack-numpy default hook: ndarrays and numpy scalars as {nd, type, kind, shape, data}."""
    if isinstance(o, np.ndarray):
        return {"nd": True, "type": o.dtype.str, "kind": "", "shape": list(o.shape), "data": np.ascontiguousarray(o).tobytes()}
    if isinstance(o, np.generic):
        return {"nd": False, "type": o.dtype.str, "data": o.tobytes()}
    raise TypeError(f"cannot serialise {type(o)}")


def read_scene(path):
    """One ``*.msgpack.zst`` file -> list of per-frame dicts (run_sample.py:200-205, Dataset.__getitem__ :199-207)."""
    with open(path, "rb") as f:
        return msgpack.unpackb(zstd_decompress(f.read()), raw=False, object_hook=_decode, strict_map_key=False)


def write_scene(path, frames, level=19):
    """Inverse of :func:`read_scene` (the cache writer of DatasetGroup.gen_data :168-176)."""
    with open(path, "wb") as f:
        f.write(zstd_compress(msgpack.packb(frames, use_bin_type=True, default=_encode), level))


class Dataset:
    """datasets/dataset_reader_physics.py:179-207."""

    def __init__(self, data=None, dataset_path=None):
        self.data, self.files = None, None
        if dataset_path is not None:
            self.files = sorted(glob.glob(os.path.join(dataset_path, "*.msgpack.zst")))
            assert len(self.files), "List of files must not be empty"
        elif data is not None:
            self.data = data
        else:
            raise NotImplementedError()

    def __len__(self):
        return len(self.data) if self.data is not None else len(self.files)

    def __getitem__(self, idx):
        return self.data[idx] if self.data is not None else read_scene(self.files[idx])


class DatasetGroup:
    """datasets/dataset_reader_physics.py:85-142: ``dataset_path`` holds the scene files (``*.msgpack.zst``) of the split, in
    ``<path>/test`` (``<path>/valid``) if that directory exists, else in ``<path>`` itself; ``split="train"`` reads
    ``<path>/train`` as well.  ``data``: scenes already in memory (a list of per-scene frame lists, e.g. a committed fixture),
    then every split, train included, is that data.  The training-side generators
    (``type: column | free_fall`` without a dataset_path: the reference's own 1-D SPH solver, column_gen.py) are host code
    outside the per-step hot path and are not rebuilt here: pass ``data`` or a ``dataset_path``."""

    def __init__(self, train=None, valid=None, test=None, split="train", regen=False, data=None, **dataset_cfg):
        self.name = dataset_cfg.pop("name", "dataset")
        self.train = self.valid = self.test = None
        if data is not None:
            self.test = self.valid = self.train = Dataset(data=data)
            return
        if "dataset_path" not in dataset_cfg or dataset_cfg["dataset_path"] is None:
            raise NotImplementedError(
                f"dataset type {dataset_cfg.get('type', 'tank')!r} is generated by the reference's training-side solver "
                "(datasets/column_gen.py / free_fall_gen.py), which is outside the hot path: pass --dataset_path with "
                "scene files, or DatasetGroup(data=...)")
        path = dataset_cfg.pop("dataset_path")
        if split == "train":  # :116-120
            sub = os.path.join(path, "train")
            if not os.path.exists(sub):
                # the reference raises FileNotFoundError here; NotImplementedError is what this package raised for the train
                # split before the training loop existed, and callers (and tests) catch that type
                raise NotImplementedError(f"--split train needs the training scenes in {sub} (a directory of *.msgpack.zst "
                                          "files): it does not exist")
            self.train = Dataset(dataset_path=sub)
        if split != "valid":  # :132-142
            sub = os.path.join(path, "test")
            self.test = Dataset(dataset_path=sub if os.path.exists(sub) else path)
            if split == "test":
                self.valid = self.test
        if split != "test":  # :122-127
            sub = os.path.join(path, "valid")
            self.valid = Dataset(dataset_path=sub if os.path.exists(sub) else path)


def align_vector(v0, v1):
    """Rotation taking v1 to v0 (:35-49), float32 like the reference's numpy code."""
    v0 = np.asarray(v0, dtype=np.float32)
    v1 = np.asarray(v1, dtype=np.float32)
    v0 = v0 / np.linalg.norm(v0)
    v1 = v1 / np.linalg.norm(v1)
    v = np.cross(v0, v1)
    c = np.dot(v0, v1)
    s = np.linalg.norm(v)
    if s < 1e-6:
        return (np.eye(3) * c).astype(np.float32)
    vx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=np.float32)
    return (np.eye(3, dtype=np.float32) + vx + vx @ vx * ((1 - c) / (s * s))).astype(np.float32)


def get_rollout(dataset, stride=1, time_start=0, time_end=None, random_start=1, cnt=None, translate=None, scale=None,
                grav_eqvar=None, **kwargs):
    """:410-456 with PhysicsSimDataFlow(window=0) unrolled: one dict per scene with the selected frames stacked --
    ``pos / vel / grav [T,N,3]``, ``m / viscosity [T,N]``, ``frame_id / scene_id [T]``, ``box / box_normals [T,M,3]``
    (the static boundary of frame 0 repeated, :333-341) -- after the input transform of :276-293.  Scenes whose
    particle count changes over time cannot be stacked (as in the reference).  ``random_start > 1`` (:428-435): one
    offset per scene from ``np.random.randint(random_start * stride)`` shifts both ends of the frame window (the validation
    split's configs use it; run_pipeline seeds numpy with 42)."""
    out = []
    for si in range(len(dataset)):
        if cnt is not None and len(out) >= cnt:
            break
        off = np.random.randint(random_start * stride) if random_start > 1 else 0
        frames = dataset[si]
        sel = [f for f in frames
               if int(f["frame_id"]) >= time_start * stride + off and int(f["frame_id"]) % stride == 0
               and (time_end is None or int(f["frame_id"]) < time_end * stride + off)]
        if not sel:
            continue
        merge = {}
        for k in ("pos", "vel", "grav", "m", "viscosity"):
            if k in sel[0] and sel[0][k] is not None:
                merge[k] = np.stack([np.asarray(f[k], dtype=np.float32) for f in sel], 0)
        for k in ("box", "box_normals"):
            b = np.asarray(frames[0][k], dtype=np.float32).reshape(-1, 3) if k in frames[0] else np.empty((0, 3), np.float32)
            merge[k] = np.stack([b for _ in sel], 0)
        merge["frame_id"] = np.asarray([f["frame_id"] for f in sel])
        merge["scene_id"] = np.asarray([f.get("scene_id", "") for f in sel])
        if "grav" in merge:
            merge["grav"] = np.broadcast_to(merge["grav"].reshape(len(sel), 1, 3), merge["vel"].shape).copy()  # :349-353
        if translate is not None:  # :276-293
            merge["pos"] = merge["pos"] + np.float32(translate)
            merge["box"] = merge["box"] + np.float32(translate)
        if scale is not None:
            for k in ("pos", "box", "vel", "grav"):
                if k in merge:
                    merge[k] = merge[k] * np.float32(scale)
        if grav_eqvar is not None and "grav" in merge:
            R = align_vector(grav_eqvar, merge["grav"][0, 0])
            merge["orig_grav"] = merge["grav"][0, 0].copy()
            for k in ("box", "box_normals", "pos", "vel", "grav"):
                merge[k] = np.matmul(merge[k], R)
        out.append(merge)
    return out


def random_rotation_matrix(rot_axis=None, dtype=np.float32, rng=np.random):
    """:52-78 with ``rot_axis`` (the shipped configs' form: Liquid3d's ``rotate: {rot_axis: 1}``): a rotation by
    theta = 2 pi x[0] about that axis, x = rng.rand(3) (the global numpy generator, as in the reference).  The reference's
    branch without an axis reads an undefined ``strength`` and cannot run; it raises here."""
    x = rng.rand(3)
    theta = x[0] * 2 * np.pi
    st, ct = np.sin(theta), np.cos(theta)
    if rot_axis is None:
        raise NotImplementedError("augment rotate without rot_axis (the reference's branch references an undefined 'strength')")
    if rot_axis == 0:
        return np.array([[1, 0, 0], [0, ct, st], [0, -st, ct]]).astype(dtype)
    if rot_axis == 1:
        return np.array([[ct, 0, st], [0, 1, 0], [-st, 0, ct]]).astype(dtype)
    return np.array([[ct, st, 0], [-st, ct, 0], [0, 0, 1]]).astype(dtype)


class PhysicsSimDataFlow:
    """:210-357: training samples of a :class:`Dataset`.  For every scene (shuffled with ``shuffle``) and every start frame
    ``i`` in ``range(len(scene) - (window + pre_frames) * stride)`` (shuffled, the first ``sample_cnt`` kept) one sample of
    ``pre + window + 1`` frames ``i, i + stride, ...`` with ``pre = np.random.randint(pre_frames + 1)``: ``pos / vel / grav /
    m / viscosity`` stacked [T, N, ...] (``[None]`` when a frame lacks the key), ``grav`` broadcast to every particle,
    ``box / box_normals`` frame 0's repeated [T, M, 3], ``frame_id / scene_id``, ``pre``; then :meth:`transform`.

    Random numbers: the scene / frame shuffles and the jitter come from ``self.rng`` (np.random.RandomState(seed)); ``pre`` and
    the rotation from the global numpy generator, as in the reference (run_pipeline seeds it with 42)."""

    def __init__(self, dataset, shuffle=False, window=1, is2d=False, pre_frames=0, stride=1, sample_cnt=None, augment=None,
                 translate=None, scale=None, grav_eqvar=None, seed=0, **kwargs):
        assert window >= 0
        self.dataset = dataset
        self.shuffle = shuffle
        self.window = window + 1
        self.is2d = is2d
        self.pre_frames = pre_frames
        self.stride = stride
        self.augment = augment or {}
        self.translate = translate
        self.grav_eqvar = grav_eqvar
        self.scale = scale
        self.sample_cnt = sample_cnt
        self.rng = np.random.RandomState(seed)

    def transform(self, data):
        """:240-293: the augment modes in config order, then translate / scale / grav_eqvar."""
        for mode, config in self.augment.items():
            config = config or {}
            if mode == "rotate":
                rand_R = random_rotation_matrix(**config)
                for k in ["box", "box_normals", "pos", "vel"]:
                    data[k] = np.matmul(data[k], rand_R)
                if data["grav"][0] is not None:
                    # the reference writes the rotated gravity to data[k], k leaked from the loop above: 'vel' is REPLACED
                    # by the rotated gravity and 'grav' stays unrotated (:247-248, restated as written)
                    data[k] = np.matmul(data["grav"], rand_R)
            elif mode == "jitter":
                for k, v in config["channels"].items():
                    data[k] += self.rng.normal(scale=v, size=data[k].shape)
            elif mode == "jitter_inp":
                for k, v in config["channels"].items():
                    data[k][0] += self.rng.normal(scale=v, size=data[k][0].shape)
            else:
                raise NotImplementedError(mode)
        if self.translate is not None:
            data["pos"] += self.translate
            data["box"] += self.translate
        if self.scale is not None:
            data["pos"] *= self.scale
            data["box"] *= self.scale
            data["vel"] *= self.scale
            if data["grav"][0] is not None:
                data["grav"] *= self.scale
        if self.grav_eqvar is not None:
            R = align_vector(self.grav_eqvar, data["grav"][0, 0])
            data["orig_grav"] = data["grav"][0, 0]
            for k in ["box", "box_normals", "pos", "vel", "grav"]:
                data[k] = np.matmul(data[k], R)
        return data

    def __iter__(self):
        files_idxs = np.arange(len(self.dataset))
        if self.shuffle:
            self.rng.shuffle(files_idxs)
        for file_i in files_idxs:
            data = self.dataset[file_i]
            data_idxs = np.arange(len(data) - (self.window - 1 + self.pre_frames) * self.stride)
            assert len(data_idxs) > 0
            if self.shuffle:
                self.rng.shuffle(data_idxs)
            if self.sample_cnt is not None:
                data_idxs = data_idxs[:self.sample_cnt]
            for data_i in data_idxs:
                sample = {"pre": np.random.randint(self.pre_frames + 1)}
                frames = range(sample["pre"] + self.window)
                for k in ["pos", "vel", "grav", "m", "viscosity"]:
                    if k in data[data_i]:
                        sample[k] = np.stack([np.asarray(data[data_i + i * self.stride].get(k, None)).astype("float32")
                                              for i in frames], 0)
                    else:
                        sample[k] = [None]
                for k in ["box", "box_normals"]:
                    if k in data[0]:
                        sample[k] = np.stack([np.asarray(data[0].get(k, None)).astype("float32") for i in frames], 0)
                    else:
                        sample[k] = [np.empty((0, 3))]
                    sample[k] = np.reshape(sample[k], (len(sample[k]), -1, 3))
                for k in ["frame_id", "scene_id"]:
                    sample[k] = np.stack([data[data_i + i * self.stride].get(k, None) for i in frames], 0)
                if sample["grav"][0] is not None:
                    sample["grav"] = np.full_like(sample["vel"], np.expand_dims(sample["grav"], 1))
                yield self.transform(sample)


def get_dataloader(dataset, batch_size=1, window=1, repeat=False, shuffle_buffer=None, num_workers=1, cache_data=False,
                   is2d=False, pre_frames=0, stride=1, translate=None, scale=None, augment=None, seed=0, **kwargs):
    """:469-517 -> an iterator of batches: dicts of per-sample lists (tensorpack's BatchData(use_list=True); an incomplete
    last batch is dropped).  ``repeat``: the flow restarts when exhausted; ``shuffle_buffer``: the samples pass a local
    shuffle buffer of that many entries (seeded: ``seed``), and the flow shuffles scenes and start frames.  ``num_workers``
    is accepted and ignored: samples are produced in this process (the reference's MultiProcessRunnerZMQ workers are not
    ported); ``cache_data`` likewise.  Samples stay numpy arrays (the reference's to_tensor happens in the training step)."""
    df = PhysicsSimDataFlow(dataset=dataset, shuffle=bool(shuffle_buffer), window=window, is2d=is2d, pre_frames=pre_frames,
                            stride=stride, augment=augment, translate=translate, scale=scale, seed=seed, **kwargs)
    rng = np.random.RandomState(seed + 1)

    def samples():
        while True:
            yield from df
            if not repeat:
                return

    def shuffled():
        if not shuffle_buffer:
            yield from samples()
            return
        # tensorpack's LocallyShuffleData, simplified: fill a buffer of shuffle_buffer samples, then hand out a random entry
        # of it for every new sample that comes in (and drain it in random order at the end of a finite flow)
        buf = []
        for s in samples():
            if len(buf) < shuffle_buffer:
                buf.append(s)
                continue
            j = rng.randint(len(buf))
            out, buf[j] = buf[j], s
            yield out
        while buf:
            yield buf.pop(rng.randint(len(buf)))

    def batches():
        batch = []
        for s in shuffled():
            batch.append(s)
            if len(batch) == batch_size:
                yield {k: [b[k] for b in batch] for k in batch[0]}
                batch = []

    return batches()


def write_results(path, name, data):
    """:520-526: HDF5 file with one group ``name`` and one dataset per (array, props) entry, attrs ``type`` / ``dim``
    -- what utils/draw_sim2d.py:170-174 reads.  Written through h5py when that is installed (the reference's own call
    sequence), otherwise by the built-in writer (dmcf_amd/utils/hdf5_writer.py: contiguous little-endian datasets in a
    version-0 HDF5 file; checked against the HDF5 C library in tests/test_hdf5_writer.py)."""
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None:
        with h5py.File(os.path.join(path), "w") as f:
            grp = f.create_group(name)
            for d, props in data:
                dset = grp.create_dataset(props["name"], data=d)
                dset.attrs["type"] = props.get("type", "DENSITY")
                dset.attrs["dim"] = d.shape
        return
    from ..utils.hdf5_writer import write_hdf5
    write_hdf5(os.path.join(path), name,
               [(props["name"], np.asarray(d), {"type": props.get("type", "DENSITY"), "dim": np.asarray(np.shape(d), dtype=np.int64)})
                for d, props in data])


def write_results_npz(path, name, data):
    """Same content as :func:`write_results` in a numpy archive: ``<name>/<dataset>`` arrays and ``<name>/<dataset>.type``."""
    arrays = {}
    for d, props in data:
        arrays[f"{name}/{props['name']}"] = np.asarray(d)
        arrays[f"{name}/{props['name']}.type"] = np.asarray(props.get("type", "DENSITY"))
    np.savez_compressed(path, **arrays)
