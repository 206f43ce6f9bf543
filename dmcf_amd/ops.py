"""Operator surface of the hot path on MI355X -- the stand-in for ``open3d.ml.tf`` (``ml3d``).

Same names, argument meaning and error behaviour as the Open3D operators the reference calls
(paths relative to the reference tree):

  ml3d.layers.FixedRadiusSearch    utils/convolutions.py:207-210 (ctor), :354-358 (call),
                                   utils/tools/losses.py:296-298 (tuple-unpacked)
  ml3d.layers.RadiusSearch         utils/convolutions.py:212-216 (ctor), :366-370, :1006-1010 (call)
  ml3d.ops.continuous_conv         utils/convolutions.py:414-431, :454
  ml3d.ops.reduce_subarrays_sum    models/pbf_model.py:450-453

Tensors are torch CUDA (= ROCm) tensors; torch is only plumbing here (device memory, streams).
All arithmetic happens in libdmcf_hip.so through its C ABI (include/dmcf_hip.h).  There is no CPU
fallback: calling these with CPU tensors or without the built library raises.
"""
import collections
import functools
import os
import ctypes

import threading

import numpy as np
import torch

from . import _lib

class NeighborCapacityExceeded(RuntimeError):
    """A search enqueued with estimated buffer sizes produced more pairs than the buffers hold."""


class NeighborSearchResult:
    """(neighbors_index int32 [P], neighbors_row_splits int64 [m+1], neighbors_distance float32 [P]) as returned by
    ``ml3d.layers.FixedRadiusSearch`` -- attribute access and tuple unpacking both work
    (utils/convolutions.py:381-382, utils/tools/losses.py:297-298).

    The index / distance buffers may be LARGER than P when the search was enqueued without a host round trip
    (``capacity_hint``); the public attributes then synchronise once and return exact-length views.  Internal
    consumers use :meth:`raw`, which never synchronises (the kernels only need row_splits)."""

    def __init__(self, index_buf, row_splits, dist_buf, total=None, redo=None):
        self._index_buf, self._dist_buf = index_buf, dist_buf
        self.neighbors_row_splits = row_splits
        self._total = total
        self._redo = redo

    def raw(self):
        return self._index_buf, self.neighbors_row_splits, self._dist_buf

    def release(self):
        """Drop the index / distance buffers (the per-step neighbour cache calls this once a list's last consumer has
        enqueued its kernel: a 3e8-pair list is 2.4 GB, padded 3.4 GB).  Row splits / counts stay."""
        if self._index_buf is not None:
            self._capacity = self._index_buf.shape[0]  # (still needed to validate an estimated size at the end of the step)
        self._index_buf = self._dist_buf = None
        self._redo = None

    @property
    def total_ref(self):
        """0-dim device tensor holding P (no synchronisation)."""
        return self.neighbors_row_splits[-1]

    @property
    def capacity(self):
        return self._index_buf.shape[0] if self._index_buf is not None else self._capacity

    def resolve(self):
        """Make the result exact: one synchronisation; repeats the write pass if the estimate was too small."""
        if self._total is None:
            total = int(self.neighbors_row_splits[-1].item())
            if total > self._index_buf.shape[0]:
                self._index_buf, self._dist_buf = self._redo(pair_capacity(total))
            self._total = total
        return self._total

    def overflowed(self, total):
        return self._total is None and total > self.capacity

    @property
    def neighbors_index(self):
        return self._index_buf[:self.resolve()]

    @property
    def neighbors_distance(self):
        n = self.resolve()
        return self._dist_buf[:n] if self._dist_buf.shape[0] >= n else self._dist_buf

    def __iter__(self):
        return iter((self.neighbors_index, self.neighbors_row_splits, self.neighbors_distance))

    def __getitem__(self, i):
        return tuple(self)[i]

    def __len__(self):
        return 3

class PaddedNeighborList(NeighborSearchResult):
    """Result of the single-pass search (dmcf_frs_search_padded): row i lives at ``index[i * stride ...]`` with
    ``counts[i]`` entries; no count pass, no prefix scan, no host round trip.  ``raw()`` / ``row_count`` feed the
    kernels directly; the Open3D-style attributes compact the rows on first use (one synchronisation)."""

    def __init__(self, index_buf, row_begin, dist_buf, counts, max_count, stride, redo_exact):
        super().__init__(index_buf, row_begin, dist_buf, total=None, redo=None)
        self.row_count = counts          # int32 [m]
        self.max_count = max_count       # int32 [1] on the device: largest unclamped row
        self.stride = int(stride)
        self._redo_exact = redo_exact
        self._compact = None

    @property
    def total_ref(self):
        """0-dim device tensor holding P (no synchronisation); summed once per list, not once per consumer."""
        t = getattr(self, "_total_ref", None)
        if t is None:
            # (an int32 tensor summed into int64 costs a cast launch and the reduction; rows x stride bounds the total on the host)
            small = self.row_count.shape[0] * self.stride < 2 ** 31
            t = self._total_ref = self.row_count.sum(dtype=torch.int32) if small else self.row_count.sum()
        return t

    def release(self):
        super().release()
        self._redo_exact = None
        self._compact = None

    def overflowed(self, max_count):
        return max_count > self.stride

    def resolve(self):
        if self._compact is None:
            if int(self.max_count.item()) > self.stride:  # truncated rows: the exact two-pass search instead
                self._compact = self._redo_exact()
            else:
                m = self.row_count.shape[0]
                cnt = self.row_count.long()
                rs = torch.zeros(m + 1, dtype=torch.int64, device=cnt.device)
                torch.cumsum(cnt, 0, out=rs[1:])
                total = int(rs[-1].item())
                row = torch.repeat_interleave(torch.arange(m, device=cnt.device), cnt, output_size=total)
                src = row * self.stride + (torch.arange(total, device=cnt.device) - rs[:-1][row])
                dist = self._dist_buf[src] if self._dist_buf.shape[0] else self._dist_buf
                self._compact = NeighborSearchResult(self._index_buf[src], rs, dist, total=total)
        return self._compact

    @property
    def neighbors_index(self):
        return self.resolve().neighbors_index

    @property
    def neighbors_distance(self):
        return self.resolve().neighbors_distance

    @property
    def csr_row_splits(self):
        return self.resolve().neighbors_row_splits

    def __iter__(self):
        c = self.resolve()
        return iter((c.neighbors_index, c.neighbors_row_splits, c.neighbors_distance))


MAPPINGS = {"ball_to_cube_radial": 0, "ball_to_cube_volume_preserving": 1, "identity": 2}
INTERPOLATIONS = {"linear": 0, "linear_border": 1, "nearest_neighbor": 2}
WINDOWS = {None: 0, "explicit": 1, "poly6": 2, "cubic": 3, "linear": 4, "peak": 5, "cubic_grad": 6}

FLAG_ALIGN_CORNERS, FLAG_NORMALIZE, FLAG_SYMMETRIC, FLAG_ACCUMULATE, FLAG_SKIP_SELF, FLAG_FILTER_PACKED = 1, 2, 4, 8, 16, 32  # DMCF_FLAG_*


class LaunchTimer:
    """Optional per-launch timing with HIP events on the stream the kernels are enqueued on (torch's current
    stream).  bench.py installs one to measure the CConv kernel's average launch duration inside the timed
    region; when ``ops.timer`` is None (the default) nothing is recorded."""

    def __init__(self):
        self.records = []  # (kind, meta dict, start event, end event)

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    def end(self, kind, meta, start):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        self.records.append((kind, meta, start, ev))

    def results(self):
        """-> list of (kind, meta, milliseconds); call after a device synchronise."""
        out = []
        for k, m, s, e in self.records:
            m = {a: (int(b.item()) if isinstance(b, torch.Tensor) else b) for a, b in m.items()}
            out.append((k, m, s.elapsed_time(e)))
        return out


timer = None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    # (the raw handle of torch's current stream: ~1 us; torch.cuda.current_stream() builds a Stream object, 12 us, and a
    # step of the 2-D models asks 80 times)
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_f32(t, name, cols=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if not t.is_cuda:
        raise _lib.DmcfError(f"{name} is on {t.device}: the DMCF hot path runs on the GPU only (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise ValueError(f"{name} must have shape [n,{cols}], got {tuple(t.shape)}")
    t = t.contiguous()
    if t.data_ptr() % 16:  # the kernels use 16-byte vector loads on feature / filter rows
        t = t.clone()
    return t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _workspace(device, query, *args, least=1):
    """The scratch buffer of one call -> (uint8 tensor, bytes to pass with it).  ``query``: the name of the entry point's
    ``*_workspace_bytes`` function, ``args`` its arguments.  The tensor has at least ``least`` bytes: a query that answers 0
    still gives the call a pointer that is not NULL."""
    nbytes = int(getattr(_lib.lib(), query)(*args))
    return torch.empty(max(nbytes, least), dtype=torch.uint8, device=device), nbytes


class SpatialHashTable:
    """Result of :func:`build_spatial_hash_table`: the cell-sorted grid of one point set for one radius.

    Plays the role of Open3D's (hash_table_index, hash_table_cell_splits, hash_table_splits) triple,
    which the reference can pass as ``fixed_radius_search_hash_table`` (utils/convolutions.py:283,358).
    """

    def __init__(self, points, radius, workspace, n_queries_capacity, row_splits=None, row_splits_dev=None):
        self.points = points
        self.radius = float(radius)
        self.workspace = workspace
        self.n_queries_capacity = n_queries_capacity
        # a batched structure (dmcf_frs_build_batched) remembers the points_row_splits it was built with: a tuple of ints
        # and the device copy the kernels read; None for the structure of one point set
        self.row_splits = row_splits
        self.row_splits_dev = row_splits_dev


def _host_row_splits(row_splits, name):
    """Row splits as given (a sequence, a CPU int64 tensor or a device int64 tensor) -> (tuple of ints, the device tensor or
    None).  A device tensor is read back here: one small synchronising copy."""
    dev = None
    if isinstance(row_splits, RowSplits):  # (both forms at hand: no copy in either direction)
        return tuple(row_splits.host), row_splits.dev
    if isinstance(row_splits, torch.Tensor):
        if row_splits.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {row_splits.dtype}")
        if row_splits.dim() != 1:
            raise ValueError(f"{name} must have rank 1, got shape {tuple(row_splits.shape)}")
        if row_splits.is_cuda:
            dev = row_splits.contiguous()
        host = tuple(row_splits.tolist())
    else:
        host = tuple(int(v) for v in row_splits)
        if any(h != v for h, v in zip(host, row_splits)):
            raise ValueError(f"{name} must hold integers")
    return host, dev


def _check_row_splits(host, total, name):
    """ValueError unless `host` starts at 0, does not decrease, ends at `total` and has at least 2 entries."""
    if len(host) < 2:
        raise ValueError(f"{name} must have at least 2 entries (batch + 1), got {len(host)}")
    if host[0] != 0:
        raise ValueError(f"{name} must start at 0, got {host[0]}")
    if any(b < a for a, b in zip(host, host[1:])):
        raise ValueError(f"{name} must not decrease")
    if host[-1] != total:
        raise ValueError(f"{name} must end at the number of rows ({total}), got {host[-1]}")


def _batched_row_splits(points, queries, points_row_splits, queries_row_splits):
    """The host-side checks of a batched search, in the order the callers rely on -- all of them before a device is touched:
    both or neither (NotImplementedError), then well-formed (ValueError).  -> ((host, dev), (host, dev))."""
    if points_row_splits is None or queries_row_splits is None:
        raise NotImplementedError("batched search needs both points_row_splits and queries_row_splits")
    p = _host_row_splits(points_row_splits, "points_row_splits")
    q = _host_row_splits(queries_row_splits, "queries_row_splits")
    _check_row_splits(p[0], points.shape[0], "points_row_splits")
    _check_row_splits(q[0], queries.shape[0], "queries_row_splits")
    if len(p[0]) != len(q[0]):
        raise ValueError(f"points_row_splits and queries_row_splits must have equal lengths (batch + 1), got {len(p[0])} and {len(q[0])}")
    return p, q


def _row_splits_on(host, dev, device):
    return dev if dev is not None and dev.device == device else torch.tensor(host, dtype=torch.int64, device=device)


def build_spatial_hash_table(points, radius, n_queries=None, points_row_splits=None, **_ignored):
    """ml3d.ops.build_spatial_hash_table equivalent (hash_table_size_factor etc. are accepted and ignored:
    the structure is a dense cell-sorted grid, see dmcf_amd/csrc/frs.hip).

    ``points_row_splits`` (a sequence, a CPU or a device int64 tensor; a device tensor costs one small synchronising copy for
    its validation): the structure of a BATCH of point sets (dmcf_frs_build_batched), which remembers its splits and serves
    searches with those splits only."""
    host = rs_dev = batch = None
    if points_row_splits is not None:
        host, dev = _host_row_splits(points_row_splits, "points_row_splits")
        _check_row_splits(host, points.shape[0], "points_row_splits")
        batch = len(host) - 1
    points = _dev_f32(points, "points", 3)
    n = points.shape[0]
    m = n if n_queries is None else int(n_queries)
    nbytes = _frs_workspace_bytes(n, m, batch)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    if batch is not None:
        rs_dev = _row_splits_on(host, dev, points.device)
    t0 = timer.begin() if timer is not None else None
    if batch is None:
        _lib.call("dmcf_frs_build", _ptr(points), n, float(radius), _ptr(ws), nbytes, _stream())
        kind, meta = "frs_build", dict(n_points=n)
    else:
        _lib.call("dmcf_frs_build_batched", _ptr(points), n, _ptr(rs_dev), batch, float(radius), _ptr(ws), nbytes, _stream())
        kind, meta = "frs_build_batched", dict(n_points=n, batch=batch)
    if timer is not None:
        timer.end(kind, meta, t0)
    return SpatialHashTable(points, radius, ws, m, row_splits=host, row_splits_dev=rs_dev)


def _frs_workspace_bytes(n, m, batch=None):
    """Bytes of the search structure of n points with room for m queries; ``batch``: items of a batched one, else None."""
    L = _lib.lib()
    return L.dmcf_frs_workspace_bytes(n, m) if batch is None else L.dmcf_frs_workspace_bytes_batched(n, m, batch)


def _serving_table(hash_table, points, radius, m, p_splits=None):
    """The caller's ``hash_table`` when it is the structure of exactly these points, this radius and these points_row_splits
    with room for m queries, else a new one.  ``p_splits``: the (host, dev) pair of the points' row splits, None for a single
    point set -- which a batched structure does not serve, nor the other way round."""
    host, dev = p_splits if p_splits is not None else (None, None)
    if (hash_table is None or hash_table.n_queries_capacity < m or hash_table.points.data_ptr() != points.data_ptr()
            or hash_table.radius != radius or hash_table.row_splits != host):
        hash_table = build_spatial_hash_table(points, radius, n_queries=m, points_row_splits=host if dev is None else dev)
    return hash_table


def reserve_device_memory(gib, device=None):
    """Make torch's caching allocator hold ONE free block of at least ``gib`` GiB (the allocator splits a cached block, it
    cannot join two segments): the multi-GB list buffers of a rollout -- and the bigger ones a scene grows into -- are then
    carved out of memory the process already owns instead of a fresh hipMalloc in the middle of a step (0.1 - 0.3 s each on
    an MI355X, with everything else queued behind it).  Optional; one GPU has 288 GB.  ``Simulator(reserve_gib=...)`` calls it.

    Returns the GiB this call took FROM THE DEVICE: ``gib`` when a new segment was created, 0.0 when the pool already held a
    free block that large (nothing to do -- the promise holds) and -1.0 when the device does not have that much to spare (the
    rollout then allocates as it goes)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    before = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
    try:
        block = torch.empty(int(gib * (1 << 30)), dtype=torch.uint8, device=dev)
    except torch.cuda.OutOfMemoryError:
        return -1.0
    del block
    return float(gib) if torch.cuda.memory_stats(dev).get("num_device_alloc", 0) > before else 0.0


def pair_capacity(total):
    """Entries to allocate for a neighbour list of ``total`` pairs: 1/8 slack (the list of the next time step fits
    the same buffer) rounded up to 1/8 of the enclosing power of two, so that a rollout asks the caching allocator
    for the same few block sizes every step instead of a slightly different one each time (each new size is a
    hipMalloc of hundreds of MB: measured 12-18 GB of fresh allocations per step until sizes happened to repeat)."""
    x = int(total) + int(total) // 8 + 65536
    return _size_class(x)


def _size_class(x):
    """Buffer sizes (in 4-byte entries) the caching allocator can hand around: 1/8 of the enclosing power of two, and from
    512 MB on whole multiples of 1 GB -- the big lists of a step then fall into two or three classes, a block freed by
    one list fits the next one exactly instead of being split, and the pool stops growing after a step or two (with finer
    classes the pool of the 1M-particle rollout was still growing -- a fresh 3 GB hipMalloc, 100 ms -- in its fifth step)."""
    x = max(int(x), 1)
    if x >= 1 << 27:
        g = 1 << 28
    else:
        g = max(1 << 16, 1 << max(x.bit_length() - 4, 0))
    return (x + g - 1) // g * g


FRS_IGNORE_QUERY_POINT, FRS_OPEN3D_CORNER_VOXELS, FRS_OPEN3D_VOXEL_WALK, FRS_METRIC_LINF = 1, 2, 4, 8  # DMCF_FRS_*

# Which neighbour SET the searches return (include/dmcf_hip.h, DMCF_FRS_*):
#   "distance"        every point with d^2 <= R^2 -- what open3d's walk over the query's own voxel and the 8 corner voxels of
#                     q +- R covers in exact arithmetic.  Symmetric lists: the ASCC head conserves
#                     momentum (models/sym_net.py:42-53).  THE DEFAULT.
#   "open3d"          that walk as float arithmetic executes it: about one query in 10^6 (a rounding step from the middle of
#                     a voxel) keeps only what lies in its own voxel; bit-exact against oracle.fixed_radius_search(bins=
#                     "own+corners"), the oracle's default.
#   "open3d_corners"  round 3's reading of the library (the 8 corner voxels alone: such a query's row is nearly empty);
#                     bit-exact against bins="corners".
# The two emulations exist so that a capture of the real library (tools/capture_golden.py) can be matched bit for bit
# whichever way it falls; they cost a fixup pass per search and break the lists' symmetry exactly where the library does.
SEARCH_SETS = {"distance": 0, "open3d": FRS_OPEN3D_VOXEL_WALK, "open3d_corners": FRS_OPEN3D_CORNER_VOXELS}


_CONSTS = {}


def const_tensor(values, dtype, device):
    """A small constant tensor on the device, built once per (values, dtype, device): ``torch.tensor(list, device=...)`` is a
    blocking host -> device copy every time -- three of them per step were a third of the synchronising calls of a 2-D model's
    step (tools/profile_small.py).  The result is shared: do not write to it."""
    key = (tuple(float(v) for v in values), dtype, str(device))
    t = _CONSTS.get(key)
    if t is None:
        if len(_CONSTS) > 256:
            _CONSTS.clear()
        t = _CONSTS[key] = torch.tensor(list(values), dtype=dtype, device=device)
    return t


def search_set():
    """The neighbour set in force: environment variable DMCF_FRS_SET (see SEARCH_SETS), "distance" when unset."""
    if "DMCF_FRS_BRUTE_FORCE_SET" in os.environ:  # (round 3's switch; silently ignoring it would run another neighbour set than asked for)
        raise ValueError("DMCF_FRS_BRUTE_FORCE_SET is gone: use DMCF_FRS_SET=distance (what it selected) | open3d | open3d_corners")
    name = os.environ.get("DMCF_FRS_SET", "distance")
    if name not in SEARCH_SETS:
        raise ValueError(f"DMCF_FRS_SET={name!r}: expected one of {sorted(SEARCH_SETS)}")
    return name


def frs_flags(ignore_query_point, batched=False):
    """Flags of the dmcf_frs_* entry points for the neighbour set in force (search_set); of the ``batched`` ones, which know the
    distance set only (their callers refuse the other sets on the host), the ignore flag alone."""
    return (FRS_IGNORE_QUERY_POINT if ignore_query_point else 0) | (0 if batched else SEARCH_SETS[search_set()])


def fixed_radius_search(points, queries, radius, ignore_query_point=False, return_distances=True,
                        hash_table=None, capacity_hint=None, row_stride=None, max_count=None, metric="L2",
                        points_row_splits=None, queries_row_splits=None):
    """-> NeighborSearchResult(neighbors_index int32 [P], neighbors_row_splits int64 [m+1],
    neighbors_distance float32 [P] (squared L2; empty if not return_distances)).

    ``metric``: "L2", or "Linf" -- the max-norm set { max_a |p_a - q_a| <= radius } of the sparse layers (DMCF_FRS_METRIC_LINF:
    the same structure and row order, index lists only: ``return_distances`` and ``row_stride`` raise, and DMCF_FRS_SET does
    not apply).

    ``capacity_hint``: an estimate of P.  With it count, scan and write are enqueued back to back with buffers of
    that size and NO host synchronisation; the result is validated later (see NeighborSearchResult).
    ``row_stride``: an upper bound of the row lengths.  With it ONE pass writes padded rows (PaddedNeighborList): no
    count pass at all; validated later through ``max_count``.
    ``points_row_splits`` / ``queries_row_splits`` (both or neither; each a sequence, a CPU int64 tensor or a device int64
    tensor -- a device tensor costs one small synchronising copy, because the splits are validated on the host): Open3D's
    batched search.  Item b of the batch is points[prs[b]:prs[b+1]] and queries[qrs[b]:qrs[b+1]]; a query finds points of its
    own item only, neighbors_index indexes the concatenated points, the row splits of the result run over all queries.  'L2'
    and DMCF_FRS_SET=distance only, no ``row_stride``; ``capacity_hint`` as without row splits."""
    batched = points_row_splits is not None or queries_row_splits is not None
    p_splits = batch = None
    if batched:
        # host checks first, in this order: both or neither; the options that have no batched form; well-formed row splits;
        # only then the operands' device
        if points_row_splits is None or queries_row_splits is None:
            raise NotImplementedError("batched search needs both points_row_splits and queries_row_splits")
        if row_stride is not None:
            raise NotImplementedError("row_stride (padded rows) has no batched form: pass row splits or row_stride, not both")
        if metric != "L2":
            raise NotImplementedError(f"metric {metric!r} has no batched form: a search with row splits is 'L2'")
        if SEARCH_SETS[search_set()] != 0:
            raise NotImplementedError(f"DMCF_FRS_SET={search_set()} has no batched form: the open3d walk emulations know nothing of items")
        p_splits, (q_host, q_dev) = _batched_row_splits(points, queries, points_row_splits, queries_row_splits)
        batch = len(q_host) - 1
    points = _dev_f32(points, "points", 3)
    queries = _dev_f32(queries, "queries", 3)
    radius = float(radius)
    if not radius > 0:
        raise ValueError("radius must be positive")
    if metric not in ("L2", "Linf"):
        raise NotImplementedError(f"metric {metric!r}: 'L2' and 'Linf' are implemented on the HIP path")
    if metric == "Linf" and (return_distances or row_stride is not None):
        raise NotImplementedError("the 'Linf' search returns index lists only (no distances, no padded rows)")
    n, m = points.shape[0], queries.shape[0]
    hash_table = _serving_table(hash_table, points, radius, m, p_splits)
    ws = hash_table.workspace
    nbytes = _frs_workspace_bytes(n, hash_table.n_queries_capacity, batch)
    flags = frs_flags(ignore_query_point)  # (a batched search runs under DMCF_FRS_SET=distance: the ignore flag alone)
    if metric == "Linf":
        flags = (FRS_IGNORE_QUERY_POINT if ignore_query_point else 0) | FRS_METRIC_LINF
    dev = points.device
    row_splits = torch.empty(m + 1, dtype=torch.int64, device=dev)
    if row_stride is not None:
        stride = max(int(row_stride), 1)
        # allocation sizes in coarse buckets (see pair_capacity): the lattice point sets change size every step
        need = m * stride
        # 1/2 headroom (HBM is plentiful: the lists of the 1M-particle scene are 9 of 288 GB): the stride moves in steps of ~9 %
        # (row_stride) while a scene compresses or heats up, and a list that outgrows its buffer asks for a fresh multi-GB
        # block -- a hipMalloc of 25-150 ms behind a drained queue in that step; run to run the driver's 20-step window of
        # the bench scene cost 73 or 83 ms per step depending on how long its three reallocations happened to take
        cap = _size_class(need + need // 2)
        # a caller that repeats this search every step passes the capacity it got last time: while that still fits (and
        # is not grossly oversized) the request stays byte-identical, and the caching allocator answers it without a
        # hipMalloc (a fresh 2 GB block costs 20-120 ms; m * stride hovers around a bucket edge for steps on end)
        if capacity_hint is not None and need <= int(capacity_hint) <= 2 * cap:
            cap = int(capacity_hint)
        elif capacity_hint is not None and need > int(capacity_hint):
            # outgrown -- a scene that is compressing or heating up keeps growing: doubling makes this reallocation the last
            # one for a long while (the rollout of the 1M-particle box outgrew 1/4 headroom five times in 25 steps)
            cap = _size_class(2 * need)
        index = torch.empty(cap, dtype=torch.int32, device=dev)
        dist = torch.empty(cap if return_distances else 0, dtype=torch.float32, device=dev)
        counts = torch.empty(m, dtype=torch.int32, device=dev)
        if max_count is None:  # (a caller with many searches per step hands out slots of ONE zeroed tensor: a fill less per search)
            max_count = torch.zeros(1, dtype=torch.int32, device=dev)
        t0 = timer.begin() if timer is not None else None  # (after the allocations: a hipMalloc is not kernel time)
        _lib.call("dmcf_frs_search_padded", _ptr(queries), m, n, radius, flags, _ptr(ws), nbytes, stride, _ptr(row_splits),
                  _ptr(counts), _ptr(index), _ptr(dist) if return_distances else None, _ptr(max_count), _stream())
        keep = (points, queries, ws)  # noqa: F841
        res = PaddedNeighborList(index, row_splits, dist, counts, max_count, stride,
                                 lambda: fixed_radius_search(points, queries, radius, ignore_query_point, return_distances,
                                                             hash_table))
        if timer is not None:
            timer.end("frs_search_padded", dict(n_points=n, n_queries=m, pairs=res.total_ref, distances=bool(return_distances)), t0)
        return res
    # one count / write body for both families: row splits select the entry points and the timer spans (frs_count and
    # frs_write around the two passes of a single point set, one frs_search_batched around both of a batch)
    if batched:
        q_rs = _row_splits_on(q_host, q_dev, dev)
        item = (_ptr(q_rs), batch)
        count, write_rows = "dmcf_frs_count_batched", "dmcf_frs_write_batched"
    else:
        q_rs, item = None, ()
        count, write_rows = "dmcf_frs_count", "dmcf_frs_write"
    t0 = timer.begin() if timer is not None else None
    _lib.call(count, _ptr(queries), m, *item, n, radius, flags, _ptr(ws), nbytes, _ptr(row_splits), _stream())
    if timer is not None and not batched:
        timer.end("frs_count", dict(n_points=n, n_queries=m), t0)

    def write(capacity):
        index = torch.empty(capacity, dtype=torch.int32, device=dev)
        dist = torch.empty(capacity if return_distances else 0, dtype=torch.float32, device=dev)
        if capacity > 0 and m > 0:
            _lib.call(write_rows, _ptr(queries), m, *item, n, radius, flags, _ptr(ws), nbytes, _ptr(row_splits), _ptr(index),
                      _ptr(dist) if return_distances else None, capacity, _stream())
        return index, dist

    if capacity_hint is None:
        total = int(row_splits[-1].item())  # the one host round trip of the two-phase search
        t1 = timer.begin() if timer is not None and not batched else t0
        index, dist = write(pair_capacity(total) if total else 0)
        res = NeighborSearchResult(index, row_splits, dist, total=total)
    else:
        t1 = timer.begin() if timer is not None and not batched else t0
        index, dist = write(pair_capacity(capacity_hint))
        keep = (points, queries, ws, q_rs)  # noqa: F841  (the closure keeps the operands alive for a possible redo)
        res = NeighborSearchResult(index, row_splits, dist, total=None, redo=write)
    if timer is not None:
        meta = dict(n_points=n, n_queries=m, pairs=res.total_ref, distances=bool(return_distances))
        if batched:
            meta["batch"] = batch
        timer.end("frs_search_batched" if batched else "frs_write", meta, t1)
    return res


class FixedRadiusSearch:
    """Mirror of ``ml3d.layers.FixedRadiusSearch`` (ctor utils/convolutions.py:207-210; call :354-358)."""

    def __init__(self, metric="L2", ignore_query_point=False, return_distances=False,
                 max_hash_table_size=32 * 2 ** 20, index_dtype=torch.int32, **kwargs):
        if metric not in ("L2", "Linf"):
            # every DMCF config uses the default radius_search_metric='L2' (utils/convolutions.py:165); the sparse layers
            # search with 'Linf' (:561-562, :760-761)
            raise NotImplementedError(f"metric {metric!r}: 'L2' and 'Linf' are implemented on the HIP path")
        if metric == "Linf" and return_distances:
            raise NotImplementedError("metric 'Linf' returns index lists only (return_distances must be False)")
        if index_dtype != torch.int32:
            raise NotImplementedError("index_dtype must be int32 (Open3D 0.15.2 returns int32 indices)")
        self.metric = metric
        self.ignore_query_point = ignore_query_point
        self.return_distances = return_distances
        self.max_hash_table_size = max_hash_table_size

    def __call__(self, points, queries, radius, points_row_splits=None, queries_row_splits=None,
                 hash_table_size_factor=1 / 64, hash_table=None, capacity_hint=None, row_stride=None, max_count=None):
        if (points_row_splits is None) != (queries_row_splits is None):  # (before anything reads a device)
            raise NotImplementedError("batched search needs both points_row_splits and queries_row_splits")
        if isinstance(radius, torch.Tensor):
            radius = float(radius)
        metric = {} if self.metric == "L2" else {"metric": self.metric}  # (an L2 call is the call it always was)
        if points_row_splits is not None or queries_row_splits is not None:  # Open3D's batched search (both or neither)
            metric.update(points_row_splits=points_row_splits, queries_row_splits=queries_row_splits)
        return fixed_radius_search(points, queries, radius, self.ignore_query_point, self.return_distances,
                                   hash_table=hash_table, capacity_hint=capacity_hint, row_stride=row_stride, max_count=max_count,
                                   **metric)

    call = __call__

    def index_only(self):
        """The same search without the distance output (for callers that re-form d^2 from the positions)."""
        twin = getattr(self, "_index_only", None)
        if twin is None:
            twin = self._index_only = FixedRadiusSearch(self.metric, self.ignore_query_point, False, self.max_hash_table_size)
        return twin


def radius_search(points, queries, radii, ignore_query_point=False, return_distances=True, normalize_distances=True,
                  points_row_splits=None, queries_row_splits=None):
    """A radius per query (dmcf_radius_search_count / _write) -> NeighborSearchResult(neighbors_index int32 [P],
    neighbors_row_splits int64 [m+1], neighbors_distance float32 [P] (empty if not return_distances)).

    Row i holds the points within ``radii[i]`` of query i (the set of include/dmcf_hip.h; always the distance set, whatever
    DMCF_FRS_SET says: the open3d emulations are of FixedRadiusSearch's hash walk).  ``normalize_distances``: d^2 / r_i^2 --
    the L2 form of Open3D's normalize_distances, restated, not pinned against the library; 0 in a row
    of radius 0.  One host read checks the radii and forms max_radius, the grid is built at max_radius, a second reads P.
    ``points_row_splits`` / ``queries_row_splits``: the batched search, as in :func:`fixed_radius_search` (both or neither,
    validated on the host before a device is touched; dmcf_radius_search_*_batched)."""
    batched = points_row_splits is not None or queries_row_splits is not None
    p_splits = batch = None
    if batched:
        p_splits, (q_host, q_dev) = _batched_row_splits(points, queries, points_row_splits, queries_row_splits)
        batch = len(q_host) - 1
    points = _dev_f32(points, "points", 3)
    queries = _dev_f32(queries, "queries", 3)
    radii = _dev_f32(radii, "radii")
    n, m = points.shape[0], queries.shape[0]
    if radii.dim() != 1 or radii.shape[0] != m:
        raise ValueError(f"radii must have shape [{m}] (one per query), got {tuple(radii.shape)}")
    dev = points.device
    row_splits = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    if m == 0:
        return NeighborSearchResult(torch.empty(0, dtype=torch.int32, device=dev), row_splits,
                                    torch.empty(0, dtype=torch.float32, device=dev), total=0)
    bad, max_radius = torch.stack([(~torch.isfinite(radii) | (radii < 0)).any().float(), radii.max()]).tolist()
    if bad:
        raise ValueError("radii must be finite and non-negative")
    max_radius = float(np.float32(max_radius)) if max_radius > 0 else 1.0  # (all zero: any grid serves, the rows are coincident points)
    flags = FRS_IGNORE_QUERY_POINT if ignore_query_point else 0
    ws = _serving_table(None, points, max_radius, m, p_splits).workspace
    nbytes = _frs_workspace_bytes(n, m, batch)
    if batched:
        q_rs = _row_splits_on(q_host, q_dev, dev)
        item = (_ptr(q_rs), batch)
        count, write = "dmcf_radius_search_count_batched", "dmcf_radius_search_write_batched"
    else:
        item = ()
        count, write = "dmcf_radius_search_count", "dmcf_radius_search_write"
    t0 = timer.begin() if timer is not None else None
    _lib.call(count, _ptr(queries), m, *item, n, _ptr(radii), max_radius, flags, _ptr(ws), nbytes, _ptr(row_splits), _stream())
    total = int(row_splits[-1].item())  # the one host round trip of the two-phase search, as in fixed_radius_search
    capacity = pair_capacity(total) if total else 0
    index = torch.empty(capacity, dtype=torch.int32, device=dev)
    dist = torch.empty(capacity if return_distances else 0, dtype=torch.float32, device=dev)
    if capacity > 0:
        _lib.call(write, _ptr(queries), m, *item, n, _ptr(radii), max_radius, flags, _ptr(ws), nbytes, _ptr(row_splits), _ptr(index),
                  _ptr(dist) if return_distances else None, capacity, _stream())
    if timer is not None:
        timer.end("radius_search", dict(n_points=n, n_queries=m, pairs=total, distances=bool(return_distances)), t0)
    if return_distances and normalize_distances and total > 0:
        r2 = radii * radii  # (float32, as the kernel's r_i * r_i)
        per_pair = torch.repeat_interleave(r2, torch.diff(row_splits), output_size=total)
        d = dist[:total]
        d.div_(per_pair).masked_fill_(per_pair == 0, 0.0)
    return NeighborSearchResult(index, row_splits, dist, total=total)


class RadiusSearch:
    """Mirror of ``ml3d.layers.RadiusSearch`` (ctor utils/convolutions.py:212-216; call :366-370, :1006-1010)."""

    def __init__(self, metric="L2", ignore_query_point=False, return_distances=False, normalize_distances=False,
                 index_dtype=torch.int32, **kwargs):
        if metric != "L2":
            raise NotImplementedError(f"metric {metric!r}: only 'L2' is implemented on the HIP path")
        if index_dtype != torch.int32:
            raise NotImplementedError("index_dtype must be int32 (Open3D 0.15.2 returns int32 indices)")
        self.metric = metric
        self.ignore_query_point = ignore_query_point
        self.return_distances = return_distances
        self.normalize_distances = normalize_distances

    def __call__(self, points, queries, radii, points_row_splits=None, queries_row_splits=None):
        if points_row_splits is not None or queries_row_splits is not None:  # Open3D's batched search (both or neither)
            return radius_search(points, queries, radii, self.ignore_query_point, self.return_distances, self.normalize_distances,
                                 points_row_splits=points_row_splits, queries_row_splits=queries_row_splits)
        return radius_search(points, queries, radii, self.ignore_query_point, self.return_distances, self.normalize_distances)

    call = __call__

    def index_only(self):
        """The same search without the distance output (for callers that re-form d^2 from the positions)."""
        twin = getattr(self, "_index_only", None)
        if twin is None:
            twin = self._index_only = RadiusSearch(self.metric, self.ignore_query_point, False, False)
        return twin


def per_point_extents(extent, n_out):
    """None for a scalar extent (a number, or a tensor of one element); else the extents as a float32 [n_out] tensor -- from
    shape [n_out] or [n_out, 1].  Anisotropic extents ([n, 3]) raise NotImplementedError, any other shape ValueError."""
    if not isinstance(extent, torch.Tensor) or extent.numel() == 1:
        return None
    if extent.dim() == 2 and extent.shape[1] == 3:
        raise NotImplementedError("anisotropic extents [n, 3] are not implemented")
    if tuple(extent.shape) not in ((n_out,), (n_out, 1)):
        raise ValueError(f"per-point extents must have shape [{n_out}] or [{n_out}, 1], got {tuple(extent.shape)}")
    return extent.reshape(n_out)


def _empty(t):
    return t is None or (isinstance(t, torch.Tensor) and t.numel() == 0)


def _extent_operands(extent, n_out):
    """``extent`` as the CConv calls take it -> (float32 device tensor [n_out] of per-point extents | None for a scalar, the
    scalar for args->extent).  Per-point extents must be finite and positive (ValueError otherwise: one host read)."""
    ext = per_point_extents(extent, n_out)
    if ext is None:
        return None, extent
    ext = _dev_f32(ext, "extents")
    if n_out > 0 and not bool((torch.isfinite(ext) & (ext > 0)).all()):
        raise ValueError("per-point extents must be finite and positive")
    return ext, 1.0  # (args->extent is ignored by the *_extents entry points; the workspace query wants a positive one)


def _kernel_name(entry, *args, size=96, checked=True):
    """The string (bytes) the ``*_kernel_name(s)`` entry point named ``entry`` writes for ``args`` into a buffer of ``size``
    bytes.  ``checked=False``: the status is not looked at (a call that fails leaves the buffer empty)."""
    name = ctypes.create_string_buffer(size)
    if checked:
        _lib.call(entry, *args, name, size)
    else:
        getattr(_lib.lib(), entry)(*args, name, size)
    return name.value


def _cconv_args(filters, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits, *,
                neighbors_value=None, window=None, window_fac=1.0, inp_importance=None, align_corners=True,
                coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", normalize=False, symmetric=False,
                sym_axis=2, bias=None, out=None, accumulate=False, neighbors_row_count=None, filter_tile_mask=0,
                skip_self=False, row_length_hint=0):
    """Validate the operands and fill a ``dmcf_cconv_args``; returns (args, keepalive tensors)."""
    filters = _dev_f32(filters, "filters")
    if filters.dim() != 5:
        raise ValueError("filters must have shape [D,H,W,Cin,Cout]")
    out_positions = _dev_f32(out_positions, "out_positions", 3)
    inp_positions = _dev_f32(inp_positions, "inp_positions", 3)
    cin, cout = filters.shape[3], filters.shape[4]
    if inp_features is not None:
        inp_features = _dev_f32(inp_features, "inp_features", cin)
        if inp_features.shape[0] != inp_positions.shape[0]:
            raise ValueError("inp_features and inp_positions disagree on the number of points")
    n_out = out_positions.shape[0]
    if neighbors_index.dtype != torch.int32 or neighbors_row_splits.dtype != torch.int64:
        raise TypeError("neighbors_index must be int32 and neighbors_row_splits int64")
    if neighbors_row_splits.shape[0] != n_out + 1:
        raise ValueError("neighbors_row_splits must have n_out+1 entries")
    if window not in WINDOWS:
        raise NotImplementedError(f"window {window!r}")
    if window is not None:
        if _empty(neighbors_value):
            if window == "explicit" and neighbors_index.numel() > 0:
                raise ValueError("explicit window but no per-neighbour values")
            neighbors_value = None  # distance windows: the kernel re-forms d^2 from the positions (as the search does)
        else:
            neighbors_value = _dev_f32(neighbors_value, "neighbors_value")
            if neighbors_value.shape[0] != neighbors_index.shape[0]:
                raise ValueError("neighbors_value and neighbors_index disagree on the number of pairs")
    inp_importance = None if _empty(inp_importance) else _dev_f32(inp_importance, "inp_importance")
    if bias is not None:
        bias = _dev_f32(bias, "bias")
    neighbors_index = neighbors_index.contiguous()
    neighbors_row_splits = neighbors_row_splits.contiguous()
    a = _lib.CconvArgs()
    a.filters = filters.data_ptr()
    for d in range(5):
        a.filter_dims[d] = filters.shape[d]
    a.sym_axis = int(sym_axis)
    a.out_positions = out_positions.data_ptr()
    a.n_out = n_out
    a.inp_positions = inp_positions.data_ptr()
    a.n_inp = inp_positions.shape[0]
    a.inp_features = None if inp_features is None else inp_features.data_ptr()
    a.inp_importance = None if inp_importance is None else inp_importance.data_ptr()
    a.neighbors_index = neighbors_index.data_ptr()
    a.neighbors_row_splits = neighbors_row_splits.data_ptr()
    a.neighbors_value = None if window is None or neighbors_value is None else neighbors_value.data_ptr()
    a.extent = float(extent)
    a.window_fac = float(window_fac)
    a.window = WINDOWS[window]
    a.coordinate_mapping = MAPPINGS[coordinate_mapping]
    a.interpolation = INTERPOLATIONS[interpolation]
    a.flags = ((FLAG_ALIGN_CORNERS if align_corners else 0) | (FLAG_NORMALIZE if normalize else 0) |
               (FLAG_SYMMETRIC if symmetric else 0) | (FLAG_ACCUMULATE if accumulate else 0) | (FLAG_SKIP_SELF if skip_self else 0))
    a.bias = None if bias is None else bias.data_ptr()
    a.out = None if out is None else out.data_ptr()
    a.n_pairs = neighbors_index.shape[0]
    a.neighbors_row_count = None
    a.filter_tile_mask = int(filter_tile_mask) & 0xffffffff
    a.row_length_hint = int(row_length_hint)
    if neighbors_row_count is not None:
        if neighbors_row_count.dtype != torch.int32 or neighbors_row_count.shape[0] != n_out:
            raise TypeError("neighbors_row_count must be int32 [n_out]")
        neighbors_row_count = neighbors_row_count.contiguous()
        a.neighbors_row_count = neighbors_row_count.data_ptr()
    keep = (neighbors_row_count, filters, out_positions, inp_positions, inp_features, inp_importance, neighbors_index, neighbors_row_splits,
            neighbors_value, bias, out)
    return a, keep


_STENCILS = {}


def lattice_offsets(voxel, radius, device, shift=(0.0, 0.0, 0.0)):
    """int32 [S, 4] device tensor: the integer offsets d (x, y, z, 0) of input cells with |d * voxel - shift| <= radius,
    decided like the search decides a pair (fp32, un-fused squared distance), ordered z, y, x."""
    return _stencil(voxel, radius, device, shift)[0]


def lattice_reach(voxel, radius, device, shift=(0.0, 0.0, 0.0)):
    """max |d| per axis (x, y, z) over :func:`lattice_offsets`: how far around the cells it covers a launch reads the input
    volume (the volume handed to :func:`lattice_conv` must be padded with zero cells that far)."""
    return list(_stencil(voxel, radius, device, shift)[1])


def _stencil(voxel, radius, device, shift):
    """(offsets, reach) of :func:`lattice_offsets` / :func:`lattice_reach`, formed once per key."""
    key = (tuple(float(v) for v in voxel), float(radius), tuple(float(v) for v in shift), str(device))
    st = _STENCILS.get(key)
    if st is None:
        v, sh = np.asarray(voxel, np.float32), np.asarray(shift, np.float32)
        reach = [int(np.floor((radius + abs(float(c))) / float(x))) + 1 if x > 0 else 0 for x, c in zip(v, sh)]
        ax = [np.arange(-r, r + 1, dtype=np.int32) for r in reach]
        dz, dy, dx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        x, y, z = dx.astype(np.float32) * v[0] - sh[0], dy.astype(np.float32) * v[1] - sh[1], dz.astype(np.float32) * v[2] - sh[2]
        d2 = (x * x + y * y) + z * z
        keep = d2 <= np.float32(radius) * np.float32(radius)
        off = np.stack([dx[keep], dy[keep], dz[keep], np.zeros(int(keep.sum()), np.int32)], axis=1).astype(np.int32)
        rch = [int(np.abs(off[:, k]).max()) if off.shape[0] else 0 for k in range(3)]
        st = (torch.from_numpy(np.ascontiguousarray(off)).to(device), rch)
        _STENCILS[key] = st
    return st


def lattice_volume_box(base_min, base_dims, inp_step, reach, points_min=None, points_dims=None):
    """(min, dims) (x, y, z) of the box of input cells a launch of :func:`lattice_conv` over the base box can touch -- its x
    extent rounded up to whole 16-cell tiles -- united with the box of the input points."""
    lo, hi = [], []
    for k in range(3):
        ext = (int(base_dims[k]) + 15) // 16 * 16 if k == 0 else int(base_dims[k])
        l = int(base_min[k]) * inp_step - int(reach[k])
        h = (int(base_min[k]) + ext - 1) * inp_step + int(reach[k])
        if points_min is not None:
            l, h = min(l, int(points_min[k])), max(h, int(points_min[k]) + int(points_dims[k]) - 1)
        lo.append(l)
        hi.append(h)
    return lo, [hi[k] - lo[k] + 1 for k in range(3)]


def _lattice_args(filters, inp_volume, inp_min, out_table, out_min, n_out, voxel, extent, *, inp_step=1, out_stride=1,
                  out_phase=(0, 0, 0), rel_shift=(0.0, 0.0, 0.0), base_min=None, base_dims=None, window="poly6", window_fac=1.0,
                  align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", bias=None,
                  out=None, accumulate=False, parts=None):
    """(ctypes array of dmcf_lattice_conv_args, one per part; tensors to keep alive; stencil offsets of all parts) of one
    call of :func:`lattice_conv` / :func:`lattice_conv_backward` (``out``: the rows written, resp. ``grad_out``)."""
    if inp_volume.dim() != 4 or inp_volume.shape[3] != filters.shape[3] or not inp_volume.is_contiguous() or not out_table.is_contiguous():
        raise ValueError("inp_volume must be a contiguous [dz, dy, dx, Cin] tensor, out_table a contiguous [dz, dy, dx] one")
    if parts is None:
        parts = [dict(out_phase=out_phase, rel_shift=rel_shift, base_min=base_min, base_dims=base_dims)]
    arr = (_lib.LatticeConvArgs * len(parts))()
    keep, n_off = [], 0
    for a, pt in zip(arr, parts):  # (a: a view of element i, so the fields are written into the array itself)
        ph, sh, bmin, bdims = pt["out_phase"], pt["rel_shift"], pt["base_min"], pt["base_dims"]
        offsets, reach = _stencil(voxel, 0.5 * float(extent), filters.device, sh)
        if bmin is None:
            bmin, bdims = out_min, [int(out_table.shape[2 - k]) for k in range(3)]
        a.filters = _ptr(filters)
        for k in range(5):
            a.filter_dims[k] = int(filters.shape[k])
        a.inp_volume, a.out_table = _ptr(inp_volume), _ptr(out_table)
        for k in range(3):
            a.inp_min[k], a.inp_dims[k] = int(inp_min[k]), int(inp_volume.shape[2 - k])
            a.out_min[k], a.out_dims[k] = int(out_min[k]), int(out_table.shape[2 - k])
            a.out_phase[k], a.base_min[k], a.base_dims[k] = int(ph[k]), int(bmin[k]), int(bdims[k])
            a.rel_shift[k], a.voxel[k], a.reach[k] = float(sh[k]), float(voxel[k]), reach[k]
        a.n_out, a.inp_step, a.out_stride = int(n_out), int(inp_step), int(out_stride)
        a.offsets, a.n_offsets = _ptr(offsets), int(offsets.shape[0])
        a.extent, a.window_fac = float(extent), float(window_fac)
        a.window = WINDOWS[window]
        a.coordinate_mapping, a.interpolation = MAPPINGS[coordinate_mapping], INTERPOLATIONS[interpolation]
        a.flags = (FLAG_ALIGN_CORNERS if align_corners else 0) | (FLAG_ACCUMULATE if accumulate else 0)
        a.bias = _ptr(bias) if bias is not None else None
        a.out = _ptr(out)
        keep.append(offsets)
        n_off += int(offsets.shape[0])
    return arr, keep, n_off


def lattice_conv(filters, inp_volume, inp_min, out_table, out_min, n_out, voxel, extent, inp_step=1, out_stride=1,
                 out_phase=(0, 0, 0), rel_shift=(0.0, 0.0, 0.0), base_min=None, base_dims=None, window="poly6",
                 window_fac=1.0, align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving",
                 interpolation="linear", bias=None, out=None, accumulate=False, fill=1.0, n_out_launch=None, parts=None):
    """dmcf_lattice_conv_forward: continuous_conv between two aligned regular lattices without a neighbour list.
    ``inp_volume`` float32 [dz, dy, dx, Cin]: the input features by cell (zeros where no point is), entry 0 = input cell
    ``inp_min`` (x, y, z), padded so that it holds every cell ``a * inp_step + d`` of the launch (:func:`lattice_volume_box`); ``out_table`` int32 [dz, dy, dx]: output point index per cell of the output lattice (-1: none),
    entry 0 = output cell ``out_min``; ``voxel`` the input lattice spacing (x, y, z).  The launch covers the output cells
    ``a * out_stride + out_phase`` for the base vectors a of the box (``base_min``, ``base_dims``; default: the whole output
    table with stride 1); their stencil is ``a * inp_step + d`` (see include/dmcf_hip.h).
    ``parts``: a list of up to 8 dicts (out_phase, rel_shift, base_min, base_dims) that replace those four arguments and
    run as ONE grid (dmcf_lattice_conv_forward_batch); every part writes rows of its own.
    While autograd records and ``filters``, ``inp_volume`` or ``bias`` requires grad, the call is a node of the graph
    (:class:`LatticeConvFunction`; ``out`` / ``accumulate`` are refused then); otherwise it is the plain forward call."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (filters, inp_volume, bias)):
        if out is not None or accumulate:
            raise ValueError("lattice_conv: out / accumulate cannot be recorded for autograd")
        geo = dict(inp_min=inp_min, out_table=out_table, out_min=out_min, n_out=n_out, voxel=voxel, extent=extent,
                   inp_step=inp_step, out_stride=out_stride, out_phase=out_phase, rel_shift=rel_shift, base_min=base_min,
                   base_dims=base_dims, window=window, window_fac=window_fac, align_corners=align_corners,
                   coordinate_mapping=coordinate_mapping, interpolation=interpolation, parts=parts)
        return LatticeConvFunction.apply(filters, inp_volume, bias, geo, dict(fill=fill, n_out_launch=n_out_launch))
    dev = filters.device
    cin, cout = filters.shape[3], filters.shape[4]
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs an out tensor")
        out = torch.zeros((n_out, cout), dtype=torch.float32, device=dev)  # rows without a cell stay 0
    filters = filters.contiguous()
    arr, keep, n_off = _lattice_args(filters, inp_volume, inp_min, out_table, out_min, n_out, voxel, extent, inp_step=inp_step,
                                     out_stride=out_stride, out_phase=out_phase, rel_shift=rel_shift, base_min=base_min,
                                     base_dims=base_dims, window=window, window_fac=window_fac, align_corners=align_corners,
                                     coordinate_mapping=coordinate_mapping, interpolation=interpolation, bias=bias, out=out,
                                     accumulate=accumulate, parts=parts)
    if len(arr) == 1:
        ws, nbytes = _workspace(dev, "dmcf_lattice_conv_workspace_bytes", arr, least=0)
    else:
        ws, nbytes = _workspace(dev, "dmcf_lattice_conv_batch_workspace_bytes", arr, len(arr), least=0)
    t0 = timer.begin() if timer is not None else None
    if len(arr) == 1:
        _lib.call("dmcf_lattice_conv_forward", arr, _ptr(ws), nbytes, _stream())
    else:
        _lib.call("dmcf_lattice_conv_forward_batch", arr, len(arr), _ptr(ws), nbytes, _stream())
    if timer is not None:
        # bench accounting: this form reads no neighbour list, so it is charged what it does read and write -- the input
        # volume once, the per-offset matrices, the cell -> point table and the output rows (``pairs_equiv`` = the pairs the
        # neighbour-list form would have had, for information only: outputs x stencil offsets x the fraction of occupied
        # cells of the input lattice's box)
        no = int(n_out if n_out_launch is None else n_out_launch)
        timer.end("cconv", dict(pairs=0, pairs_equiv=int(no * (n_off / len(arr)) * float(fill)), n_out=no, cin=int(cin),
                                cout=int(cout), K=int(filters.shape[0] * filters.shape[1] * filters.shape[2]), symmetric=False,
                                lattice=True, kernel="lat_conv_kernel", n_offsets=int(n_off), parts=len(arr),
                                volume_bytes=int(inp_volume.numel()) * 4, table_bytes=int(out_table.numel()) * 4,
                                accumulate=bool(accumulate)), t0)
    return out


def lattice_conv_backward(filters, inp_volume, inp_min, out_table, out_min, n_out, voxel, extent, grad_out, inp_step=1,
                          out_stride=1, out_phase=(0, 0, 0), rel_shift=(0.0, 0.0, 0.0), base_min=None, base_dims=None,
                          window="poly6", window_fac=1.0, align_corners=True,
                          coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", parts=None,
                          need_volume=True, need_filters=True):
    """dmcf_lattice_conv_backward: ``(grad_volume | None, grad_filters | None)`` of the convolution :func:`lattice_conv`
    computes with these arguments, for ``grad_out`` = dL/d out [n_out, Cout].  ``grad_volume`` has the shape of
    ``inp_volume`` (zero in cells no output reaches), ``grad_filters`` that of ``filters`` (summed over all ``parts``).  Rows
    of ``grad_out`` whose point is not in ``out_table`` contribute nothing.  One call of the entry point; no neighbour
    list, no inversion, no float atomics (two calls return the same bits)."""
    filters = _dev_f32(filters, "filters")
    dev = filters.device
    grad_out = _dev_f32(grad_out, "grad_out", filters.shape[4])
    if grad_out.shape[0] != n_out:
        raise ValueError("grad_out must be [n_out, Cout]")
    if not need_volume and not need_filters:
        return None, None
    arr, keep, _ = _lattice_args(filters, inp_volume, inp_min, out_table, out_min, n_out, voxel, extent, inp_step=inp_step,
                                 out_stride=out_stride, out_phase=out_phase, rel_shift=rel_shift, base_min=base_min,
                                 base_dims=base_dims, window=window, window_fac=window_fac, align_corners=align_corners,
                                 coordinate_mapping=coordinate_mapping, interpolation=interpolation, out=grad_out, parts=parts)
    gv = torch.empty_like(inp_volume) if need_volume else None
    gw = torch.empty_like(filters) if need_filters else None
    ws, nbytes = _workspace(dev, "dmcf_lattice_conv_backward_workspace_bytes", arr, len(arr), least=0)
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_lattice_conv_backward", arr, len(arr), _ptr(grad_out), _ptr(gv), _ptr(gw), _ptr(ws), nbytes, _stream())
    if timer is not None:
        timer.end("cconv_backward", dict(n_out=int(n_out), cin=int(filters.shape[3]), cout=int(filters.shape[4]),
                                         filters=bool(need_filters), features=bool(need_volume), lattice=True, parts=len(arr),
                                         kernel="lat_bwd_filter;lat_bwd_input"), t0)
    del keep
    return gv, gw


class LatticeConvFunction(torch.autograd.Function):
    """Autograd node of :func:`lattice_conv`.  It keeps the volume, the cell -> point table, the filters and the parts
    themselves (``geo``), not the lattices they came from: the per-step cache forgets those when the step ends.  The backward
    is one dmcf_lattice_conv_backward; the bias takes ``grad_out`` summed over the rows that are in the table (the rows the
    forward adds it to).  The volume's gradient reaches per-point features through the indexing that built the volume."""

    @staticmethod
    def forward(ctx, filters, inp_volume, bias, geo, info):
        ctx.geo = geo
        ctx.has_bias = bias is not None
        ctx.save_for_backward(filters, inp_volume)
        # (grad mode is off in here, so this is the plain call; a replaced ``ops.lattice_conv`` is re-entered by it)
        return lattice_conv(filters, inp_volume, bias=bias, **geo, **info)

    @staticmethod
    def backward(ctx, grad_out):
        filters, inp_volume = ctx.saved_tensors
        need_w, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        grad_out = grad_out.contiguous()
        gv, gw = lattice_conv_backward(filters.detach(), inp_volume.detach(), grad_out=grad_out, need_volume=need_v,
                                       need_filters=need_w, **ctx.geo)
        gb = None
        if need_b:
            n_out = int(ctx.geo["n_out"])
            rows = ctx.geo["out_table"].reshape(-1).long()
            hit = torch.zeros(n_out + 1, dtype=grad_out.dtype, device=grad_out.device)
            hit[torch.where(rows >= 0, rows, torch.full_like(rows, n_out))] = 1.0  # (the spare slot takes the empty cells)
            gb = (grad_out * hit[:n_out, None]).sum(0)
        return gw, gv, gb, None, None


def block_diagonal_tile_mask(blocks):
    """``filter_tile_mask`` of include/dmcf_hip.h for a filter whose only non-zero entries lie in the given blocks
    ``[(c0, c1, o0, o1), ...]`` (input channels c0 .. c1 - 1 into output channels o0 .. o1 - 1): bit 4 * (c / 4) + o / 16 for
    every (c, o) of a block.  0 (no hint) when the filter does not fit the mask (c >= 32 or o >= 64)."""
    mask = 0
    for c0, c1, o0, o1 in blocks:
        if c1 > 32 or o1 > 64:
            return 0
        for q in range(c0 // 4, (c1 + 3) // 4):
            for n in range(o0 // 16, (o1 + 15) // 16):
                mask |= 1 << (4 * q + n)
    return mask


def cconv_forward(filters, out_positions, extent, inp_positions, inp_features, neighbors_index,
                  neighbors_row_splits, neighbors_value=None, window=None, window_fac=1.0, inp_importance=None,
                  align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear",
                  normalize=False, symmetric=False, sym_axis=2, bias=None, out=None, accumulate=False,
                  n_pairs_ref=None, neighbors_row_count=None, filter_tile_mask=0, skip_self=False, name_only=False,
                  row_length_hint=0, packed_cache=None, record_per_point_extents=False):
    """One call of dmcf_cconv_forward.  ``row_length_hint``: 0 unknown / 1 tens / 2 hundreds of neighbours per row -- what the
    caller knows about the LAYER from its configuration (include/dmcf_hip.h).  ``skip_self``: DMCF_FLAG_SKIP_SELF (the list
    holds the query points, the layer ignores them; only the direct kernel).  ``name_only``: no launch, returns the name of the
    kernel these arguments dispatch to.  ``filter_tile_mask``: see ``block_diagonal_tile_mask`` (0 = no hint).
    ``neighbors_row_count``: int32 [n_out] for padded lists (PaddedNeighborList).  ``window``: None | 'explicit'
    (neighbors_value = importance) | 'poly6' | 'cubic' | 'linear' | 'peak' | 'cubic_grad' (neighbors_value = squared distances).
    ``extent``: a scalar, or one extent per output row -- a tensor of shape [n_out] or [n_out, 1] (dmcf_cconv_forward_extents:
    row i maps its pairs with extents[i] and evaluates a distance window on d^2 / (extents[i] / 2)^2).  Per-point extents must
    be finite and positive (ValueError otherwise: one host read); that call always packs the filter (``packed_cache`` unused).

    When autograd records (``torch.is_grad_enabled()``) and ``filters`` or ``inp_features`` requires grad, the call goes
    through ``CconvFunction``: the same forward kernel, and a backward through dmcf_cconv_backward.  ``bias`` is then
    differentiable too (torch adds it after the kernel).  ``out=`` / ``accumulate=True`` raise ValueError there.  Per-point
    extents (a tensor [n_out] / [n_out, 1]) record only when the caller asks for it, ``record_per_point_extents=True``: the
    backward is then dmcf_cconv_backward_extents, and the extents get no gradient (every pair is differentiated at the
    extent of its output row, which for ASCC is not the momentum-conserving layer).  Without it such a call raises
    NotImplementedError, as it always has.  Otherwise the call is exactly the inference path."""
    if not name_only and torch.is_grad_enabled() and (
            (isinstance(filters, torch.Tensor) and filters.requires_grad) or
            (isinstance(inp_features, torch.Tensor) and inp_features.requires_grad) or
            (isinstance(bias, torch.Tensor) and bias.requires_grad)):
        if out is not None or accumulate:
            raise ValueError("out= / accumulate=True cannot be recorded by autograd: use the returned tensor")
        ext = per_point_extents(extent, out_positions.shape[0])
        if ext is not None and not record_per_point_extents:
            raise NotImplementedError("recording CConv with per-point extents is opt-in: pass record_per_point_extents=True "
                                      "(the backward is dmcf_cconv_backward_extents; the extents get no gradient)")
        geo = dict(out_positions=out_positions, extent=float(extent) if ext is None else ext.detach(), inp_positions=inp_positions,
                   neighbors_index=neighbors_index, neighbors_row_splits=neighbors_row_splits, neighbors_value=neighbors_value,
                   window=window, window_fac=window_fac, inp_importance=inp_importance, align_corners=align_corners,
                   coordinate_mapping=coordinate_mapping, interpolation=interpolation, normalize=normalize, symmetric=symmetric,
                   sym_axis=sym_axis, neighbors_row_count=neighbors_row_count, skip_self=skip_self)
        res = CconvFunction.apply(filters, inp_features, geo, dict(filter_tile_mask=filter_tile_mask, row_length_hint=row_length_hint,
                                                                   n_pairs_ref=n_pairs_ref, packed_cache=packed_cache))
        if bias is not None:
            res = res + bias
        return res
    L = _lib.lib()
    n_out, cout = out_positions.shape[0], filters.shape[4]
    ext, extent = _extent_operands(extent, n_out)
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs an out tensor")
        out = torch.empty((n_out, cout), dtype=torch.float32, device=filters.device)
    elif out.shape != (n_out, cout) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out has the wrong shape / dtype / layout")
    if inp_positions.shape[0] == 0 or n_out == 0:
        # an empty input set (e.g. every boundary particle cropped away, pbf_model.py:330-336): every row is empty, the
        # result is the bias; nothing to launch (the C ABI rejects NULL point arrays)
        b = 0.0 if bias is None else bias.to(torch.float32)
        if accumulate:
            out += b
        else:
            out[:] = b
        return out
    a, keep = _cconv_args(filters, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
                          neighbors_value=neighbors_value, window=window, window_fac=window_fac, inp_importance=inp_importance,
                          align_corners=align_corners, coordinate_mapping=coordinate_mapping, interpolation=interpolation,
                          normalize=normalize, symmetric=symmetric, sym_axis=sym_axis, bias=bias, out=out, accumulate=accumulate,
                          neighbors_row_count=neighbors_row_count, filter_tile_mask=filter_tile_mask, skip_self=skip_self,
                          row_length_hint=row_length_hint)
    kernel_name = "dmcf_cconv_kernel_name" if ext is None else "dmcf_cconv_extents_kernel_name"
    if name_only:
        return _kernel_name(kernel_name, ctypes.byref(a)).decode()
    nbytes = L.dmcf_cconv_workspace_bytes(ctypes.byref(a))
    ws = None
    if packed_cache is not None and ext is None:
        # ``packed_cache``: a dict the calling LAYER owns.  It keeps the workspace of the layer's last call; while the filter
        # tensor (storage, version), its interpretation and the kernel the dispatch picks are the same, the packed filter in it
        # is still valid and is not formed again (DMCF_FLAG_FILTER_PACKED: one launch less per layer and step)
        # Identity of the filter VALUES: the tensor object itself (held by the cache, so neither its address nor its id can be
        # reused by another tensor while the entry lives) + its version counter.  In-place writes through autograd-visible
        # calls (copy_, load_state_dict, optimiser steps) bump the counter; a write through ``.data`` does not -- after one,
        # call ``layer.invalidate_packed()``.  Derived tensors (a fresh object per call) never hit.
        key = (filters._version, tuple(filters.shape), bool(symmetric), int(sym_axis),
               _kernel_name("dmcf_cconv_kernel_name", ctypes.byref(a), checked=False), str(filters.device))
        ws = packed_cache.get("ws")
        if packed_cache.get("src") is filters and packed_cache.get("key") == key and ws is not None and ws.numel() >= nbytes:
            a.flags |= FLAG_FILTER_PACKED
        else:
            # (the workspace of a small launch also holds scratch that grows with n_out: a quarter of headroom, so that a scene
            # whose point counts drift does not repack every step)
            ws = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, device=filters.device)
            packed_cache["key"], packed_cache["ws"], packed_cache["src"] = key, ws, filters
        nbytes = ws.numel()
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=filters.device)
    t0 = timer.begin() if timer is not None else None
    if ext is None:
        _lib.call("dmcf_cconv_forward", ctypes.byref(a), _ptr(ws), nbytes, _stream())
    else:
        _lib.call("dmcf_cconv_forward_extents", ctypes.byref(a), _ptr(ext), _ptr(ws), nbytes, _stream())
    if timer is not None:
        kdims = [int(d) for d in filters.shape[:3]]
        if symmetric:
            kdims[int(sym_axis)] *= 2
        timer.end("cconv", dict(pairs=n_pairs_ref if n_pairs_ref is not None else int(a.n_pairs), n_out=n_out, cin=int(filters.shape[3]), cout=cout,
                                K=kdims[0] * kdims[1] * kdims[2], symmetric=bool(symmetric), kernel=_kernel_name(kernel_name, ctypes.byref(a), checked=False).decode(),
                                pair_values=bool(a.neighbors_value), accumulate=bool(accumulate)), t0)
    return out


InvertedNeighbors = collections.namedtuple("InvertedNeighbors",
                                           ["neighbors_index", "neighbors_row_splits", "neighbors_attributes", "pair_index"])


def invert_neighbors_list(num_points, inp_neighbors_index, inp_neighbors_row_splits, inp_neighbors_attributes=None,
                          neighbors_row_count=None):
    """Mirror of ``ml3d.ops.invert_neighbors_list`` (dmcf_invert_neighbors_list): for each of the ``num_points`` input points
    the forward pairs that reference it.  Returns ``InvertedNeighbors(neighbors_index, neighbors_row_splits,
    neighbors_attributes, pair_index)``: row j of the result is ``[row_splits[j], row_splits[j+1])``, holding the OUTPUT row of
    each pair and (``pair_index``) the pair's position in the forward list, in ascending pair order.  The arrays keep the
    length of the forward list; entries past ``row_splits[-1]`` (pairs of rows reaching past the list, or of padded slots) are
    -1.  ``inp_neighbors_attributes``: None / empty or a float32 [P] tensor, returned permuted the same way.
    ``neighbors_row_count``: int32 [n_out] for padded lists, whose ``inp_neighbors_row_splits`` holds a begin per row (at
    least n_out entries)."""
    index = inp_neighbors_index
    rs = inp_neighbors_row_splits
    if index.dtype != torch.int32 or rs.dtype != torch.int64:
        raise TypeError("inp_neighbors_index must be int32 and inp_neighbors_row_splits int64")
    if not index.is_cuda or not rs.is_cuda:
        raise _lib.DmcfError("invert_neighbors_list runs on the GPU only (no CPU fallback)")
    index, rs = index.contiguous(), rs.contiguous()
    n_inp, n_out, P = int(num_points), rs.shape[0] - 1, index.shape[0]
    dev = index.device
    attrs = None if _empty(inp_neighbors_attributes) else _dev_f32(inp_neighbors_attributes, "inp_neighbors_attributes")
    if attrs is not None and attrs.shape != (P,):
        raise ValueError("inp_neighbors_attributes must be a float32 [P] tensor")
    if neighbors_row_count is not None:
        # a padded list: one row per count and a row begin for each, as neighbor_dense takes it (entries of the begins past
        # the rows, such as the end entry row splits have, are not read)
        if neighbors_row_count.dtype != torch.int32 or neighbors_row_count.dim() != 1:
            raise TypeError("neighbors_row_count must be int32 [n_out]")
        n_out = neighbors_row_count.shape[0]
        if rs.shape[0] < n_out:
            raise ValueError("padded lists need a row begin per row")
        neighbors_row_count = neighbors_row_count.contiguous()
    inv_index = torch.empty(P, dtype=torch.int32, device=dev)
    inv_pair = torch.empty(P, dtype=torch.int32, device=dev)
    inv_rs = torch.empty(n_inp + 1, dtype=torch.int64, device=dev)
    inv_attr = torch.empty(P, dtype=torch.float32, device=dev) if attrs is not None else torch.empty(0, dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(dev, "dmcf_invert_neighbors_list_workspace_bytes", P, least=0)
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_invert_neighbors_list", n_inp, _ptr(index), _ptr(rs), _ptr(neighbors_row_count), n_out, P, _ptr(attrs),
              _ptr(inv_index), _ptr(inv_rs), _ptr(inv_pair), _ptr(inv_attr) if attrs is not None else None, _ptr(ws), nbytes,
              _stream())
    if timer is not None:
        timer.end("invert", dict(pairs=P, n_inp=n_inp), t0)
    return InvertedNeighbors(inv_index, inv_rs, inv_attr, inv_pair)


def cconv_backward(filters, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits, grad_out,
                   neighbors_value=None, window=None, window_fac=1.0, inp_importance=None, align_corners=True,
                   coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", normalize=False, symmetric=False,
                   sym_axis=2, neighbors_row_count=None, skip_self=False, need_filters=True, need_features=True, inverted=None,
                   grad_filters=None, grad_inp_features=None, accumulate=False):
    """dmcf_cconv_backward: ``(grad_filters, grad_inp_features)`` of the CConv ``cconv_forward`` computes with these
    arguments, for ``grad_out`` = dL/d out [n_out, Cout].  Either can be skipped (``need_filters`` / ``need_features``
    False: None is returned for it).  ``inverted``: an ``invert_neighbors_list`` result of the same list (formed here when
    the input-feature gradient is wanted and none is given).  ``grad_filters`` / ``grad_inp_features``: output tensors to
    write, or with ``accumulate=True`` to add into.  With ``symmetric`` the filter gradient is that of the stored half
    kernel.  ``extent``: what ``cconv_forward`` accepts -- a scalar, or one extent per output row (a tensor [n_out] or
    [n_out, 1], finite and positive: ValueError otherwise), which takes dmcf_cconv_backward_extents: every pair at the extent of
    its output row.  Extents get no gradient."""
    n_out, n_inp = out_positions.shape[0], inp_positions.shape[0]
    cin = filters.shape[3]
    dev = filters.device
    ext, extent = _extent_operands(extent, n_out)
    grad_out = _dev_f32(grad_out, "grad_out", filters.shape[4])
    if grad_out.shape[0] != n_out:
        raise ValueError("grad_out must be [n_out, Cout]")
    if need_filters and grad_filters is None:
        grad_filters = (torch.zeros if accumulate else torch.empty)(tuple(filters.shape), dtype=torch.float32, device=dev)
    if need_features and grad_inp_features is None:
        grad_inp_features = (torch.zeros if accumulate else torch.empty)((n_inp, cin), dtype=torch.float32, device=dev)
    for t, shape, name in ((grad_filters if need_filters else None, tuple(filters.shape), "grad_filters"),
                           (grad_inp_features if need_features else None, (n_inp, cin), "grad_inp_features")):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"{name} must be a contiguous float32 device tensor of shape {shape}")
    if not need_filters and not need_features:
        return None, None
    a, keep = _cconv_args(filters, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
                          neighbors_value=neighbors_value, window=window, window_fac=window_fac, inp_importance=inp_importance,
                          align_corners=align_corners, coordinate_mapping=coordinate_mapping, interpolation=interpolation,
                          normalize=normalize, symmetric=symmetric, sym_axis=sym_axis, neighbors_row_count=neighbors_row_count,
                          skip_self=skip_self)
    b = _lib.CconvBackwardArgs()
    b.struct_size = ctypes.sizeof(_lib.CconvBackwardArgs)
    b.flags = 1 if accumulate else 0  # DMCF_BWD_ACCUMULATE
    b.grad_out = grad_out.data_ptr()
    if need_features:
        if inverted is None:
            inverted = invert_neighbors_list(n_inp, neighbors_index, neighbors_row_splits, None, neighbors_row_count)
        b.inv_index = inverted.neighbors_index.data_ptr()
        b.inv_pair = inverted.pair_index.data_ptr()
        b.inv_row_splits = inverted.neighbors_row_splits.data_ptr()
        b.inv_n_rows = inverted.neighbors_row_splits.shape[0] - 1
        b.inv_n_pairs = inverted.neighbors_index.shape[0]
        b.grad_inp_features = grad_inp_features.data_ptr()
    if need_filters:
        b.grad_filters = grad_filters.data_ptr()
    ws, nbytes = _workspace(dev, "dmcf_cconv_backward_workspace_bytes", ctypes.byref(a), ctypes.byref(b), least=0)
    t0 = timer.begin() if timer is not None else None
    if ext is None:
        _lib.call("dmcf_cconv_backward", ctypes.byref(a), ctypes.byref(b), _ptr(ws), nbytes, _stream())
    else:
        _lib.call("dmcf_cconv_backward_extents", ctypes.byref(a), ctypes.byref(b), _ptr(ext), _ptr(ws), nbytes, _stream())
    if timer is not None:
        timer.end("cconv_backward", dict(n_out=n_out, cin=int(cin), cout=int(filters.shape[4]), filters=bool(need_filters),
                                         features=bool(need_features),
                                         kernel=cconv_backward_kernel_names(a, b, extents=ext is not None)), t0)
    del keep
    return (grad_filters if need_filters else None), (grad_inp_features if need_features else None)


def cconv_backward_kernel_names(a, b, extents=False):
    """';'-separated names of the kernels dmcf_cconv_backward -- ``extents``: dmcf_cconv_backward_extents, whose geometry kernels
    carry the suffix _ext -- launches for these (ctypes) arguments."""
    entry = "dmcf_cconv_backward_extents_kernel_names" if extents else "dmcf_cconv_backward_kernel_names"
    return _kernel_name(entry, ctypes.byref(a), ctypes.byref(b), size=256).decode()


class CconvFunction(torch.autograd.Function):
    """Autograd node of ``cconv_forward``: the forward is whatever kernel the dispatch picks today (bias excluded: torch adds
    it); the backward is dmcf_cconv_backward (dmcf_cconv_backward_extents when ``geo["extent"]`` is a tensor of per-point
    extents, which is kept for the backward and not differentiated), with the neighbour list inverted once per backward when
    the input features want a gradient.  Positions, extents and importances get no gradient (as in Open3D)."""

    @staticmethod
    def forward(ctx, filters, inp_features, geo, info):
        ctx.geo = geo
        ctx.save_for_backward(filters, inp_features)
        # (grad mode is off in here, so this is the plain call; a replaced ``ops.cconv_forward`` is re-entered by it)
        return cconv_forward(filters, inp_features=inp_features, **geo, **info)

    @staticmethod
    def backward(ctx, grad_out):
        filters, inp_features = ctx.saved_tensors
        need_w = ctx.needs_input_grad[0]
        need_f = ctx.needs_input_grad[1] and inp_features is not None
        if not need_w and not need_f:
            return None, None, None, None
        gw, gf = cconv_backward(filters.detach(), inp_features=None if inp_features is None else inp_features.detach(),
                                grad_out=grad_out.contiguous(), need_filters=need_w, need_features=need_f, **ctx.geo)
        return gw, gf, None, None


ND_RELU, ND_W_TRANSPOSED = 1, 2  # DMCF_ND_*


class SharedInverse:
    """The inversion of one neighbour list, formed on first use and then shared: every PointNet layer of a step walks the
    same list, so its backward inverts it once per step, not once per layer.  ``n_points``: the range of the indices (the
    list's input rows); a layer with fewer input rows (PointNet's layer 0: fluid only) reads the first rows of it."""

    def __init__(self, n_points, neighbors_index, neighbors_row_splits, neighbors_row_count=None):
        self.n_points = int(n_points)
        self.args = (neighbors_index, neighbors_row_splits, neighbors_row_count)
        self._inv = None

    def get(self):
        if self._inv is None:
            index, rs, count = self.args
            self._inv = invert_neighbors_list(self.n_points, index, rs, None, count)
        return self._inv


def _nd_operands(x, kernel, bias, neighbors_index, neighbors_row_splits, n_in, residual, neighbors_row_count):
    kernel = _dev_f32(kernel, "kernel")
    if kernel.dim() != 2:
        raise ValueError("kernel must be [Cin, Cout]")
    cin, cout = kernel.shape
    x = _dev_f32(x, "x", cin)
    n_in = x.shape[0] if n_in is None else int(n_in)
    if not 0 <= n_in <= x.shape[0]:
        raise ValueError(f"n_in = {n_in} for {x.shape[0]} rows of x")
    if not isinstance(neighbors_index, torch.Tensor) or not isinstance(neighbors_row_splits, torch.Tensor):
        raise TypeError("neighbors_index and neighbors_row_splits must be torch tensors")
    if not neighbors_index.is_cuda or not neighbors_row_splits.is_cuda:
        raise _lib.DmcfError("the neighbour list is on the CPU: the DMCF hot path runs on the GPU only (no CPU fallback)")
    if neighbors_index.dtype != torch.int32 or neighbors_row_splits.dtype != torch.int64:
        raise TypeError("neighbors_index must be int32 and neighbors_row_splits int64")
    if neighbors_row_count is not None:
        if neighbors_row_count.dtype != torch.int32 or neighbors_row_count.dim() != 1:
            raise TypeError("neighbors_row_count must be int32 [n_out]")
        n_out = neighbors_row_count.shape[0]
        if neighbors_row_splits.shape[0] < n_out:
            raise ValueError("padded lists need a row begin per row")
        neighbors_row_count = neighbors_row_count.contiguous()
    else:
        n_out = neighbors_row_splits.shape[0] - 1
        if n_out < 0:
            raise ValueError("neighbors_row_splits must have n_out+1 entries")
    if bias is not None:
        bias = _dev_f32(bias, "bias")
        if tuple(bias.shape) != (cout,):
            raise ValueError("bias must be [Cout]")
    if residual is not None:
        residual = _dev_f32(residual, "residual", cout)
        if residual.shape[0] != n_out:
            raise ValueError("residual must be [n_out, Cout]")
    return (x, kernel, bias, neighbors_index.contiguous(), neighbors_row_splits.contiguous(), n_in, residual, neighbors_row_count,
            n_out, cin, cout)


def _nd_forward(x, kernel, bias, neighbors_index, neighbors_row_splits, n_in, relu, residual, neighbors_row_count, record=False):
    """dmcf_neighbor_dense_forward; returns out (and with ``record`` the aggregate S [n_out, Cin] and counts c [n_out])."""
    (x, kernel, bias, index, rs, n_in, residual, count, n_out, cin, cout) = _nd_operands(
        x, kernel, bias, neighbors_index, neighbors_row_splits, n_in, residual, neighbors_row_count)
    dev = x.device
    out = torch.empty(n_out, cout, dtype=torch.float32, device=dev)
    a = _lib.NeighborDenseArgs()
    a.struct_size = ctypes.sizeof(_lib.NeighborDenseArgs)
    a.flags = ND_RELU if relu else 0
    a.x, a.n_in, a.cin, a.cout = x.data_ptr(), n_in, cin, cout
    a.kernel = kernel.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.residual = None if residual is None else residual.data_ptr()
    a.neighbors_index, a.neighbors_row_splits = index.data_ptr(), rs.data_ptr()
    a.neighbors_row_count = None if count is None else count.data_ptr()
    a.n_out, a.n_pairs = n_out, index.shape[0]
    a.out = out.data_ptr()
    s = c = None
    if record:
        s = torch.empty(n_out, cin, dtype=torch.float32, device=dev)
        c = torch.empty(n_out, dtype=torch.float32, device=dev)
        a.record_s, a.record_count = s.data_ptr(), c.data_ptr()
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_neighbor_dense_forward", ctypes.byref(a), _stream())
    if timer is not None:
        timer.end("neighbor_dense", dict(n_out=n_out, cin=int(cin), cout=int(cout), pairs=int(index.shape[0]),
                                         kernel=neighbor_dense_kernel_names(a, None)), t0)
    return (out, s, c) if record else out


def neighbor_dense_kernel_names(fwd, bwd):
    """';'-separated names of the kernels dmcf_neighbor_dense_forward (``fwd``) and / or _backward (``bwd``) launch for these
    (ctypes) arguments."""
    return _kernel_name("dmcf_neighbor_dense_kernel_names", None if fwd is None else ctypes.byref(fwd),
                        None if bwd is None else ctypes.byref(bwd), size=256).decode()


def neighbor_dense_backward(x, kernel, grad_out, s, count, n_in=None, relu=True, inverted=None, neighbors_index=None,
                            neighbors_row_splits=None, neighbors_row_count=None, need_x=True, need_kernel=True, need_bias=True):
    """dmcf_neighbor_dense_backward: ``(grad_x, grad_kernel, grad_bias)`` of :func:`neighbor_dense` for ``grad_out`` = dL/d out,
    from the forward's recorded aggregate ``s`` and counts ``count``.  ``inverted``: an ``invert_neighbors_list`` result of the
    forward list over at least ``n_in`` input rows, or a :class:`SharedInverse`; formed from ``neighbors_index`` /
    ``neighbors_row_splits`` when None and the input gradient is wanted.  grad_x has x's rows; rows past ``n_in`` get 0."""
    kernel = _dev_f32(kernel, "kernel")
    cin, cout = kernel.shape
    x = _dev_f32(x, "x", cin)
    n_in = x.shape[0] if n_in is None else int(n_in)
    grad_out = _dev_f32(grad_out, "grad_out", cout)
    n_out = grad_out.shape[0]
    dev = x.device
    b = _lib.NeighborDenseBackwardArgs()
    b.struct_size = ctypes.sizeof(_lib.NeighborDenseBackwardArgs)
    b.flags = ND_RELU if relu else 0
    b.x, b.n_in, b.cin, b.cout = x.data_ptr(), n_in, cin, cout
    b.kernel = kernel.data_ptr()
    b.grad_out, b.n_out = grad_out.data_ptr(), n_out
    gx = gw = gb = None
    keep = []
    if need_x:
        if inverted is None:
            inverted = invert_neighbors_list(n_in, neighbors_index, neighbors_row_splits, None, neighbors_row_count)
        elif isinstance(inverted, SharedInverse):
            if inverted.n_points < n_in:
                raise ValueError("the shared inversion covers fewer input rows than the layer has")
            inverted = inverted.get()
        if inverted.neighbors_row_splits.shape[0] < n_in + 1:
            raise ValueError("the inverted list covers fewer input rows than the layer has")
        gx = torch.zeros(x.shape[0], cin, dtype=torch.float32, device=dev) if n_in < x.shape[0] else \
            torch.empty(n_in, cin, dtype=torch.float32, device=dev)
        b.inv_index = inverted.neighbors_index.data_ptr()
        b.inv_row_splits = inverted.neighbors_row_splits.data_ptr()
        b.inv_n_pairs = inverted.neighbors_index.shape[0]
        b.grad_x = gx.data_ptr()
        keep.append(inverted)
    if need_kernel or need_bias:
        s = _dev_f32(s, "s", cin)
        count = _dev_f32(count, "count")
        if s.shape[0] != n_out or tuple(count.shape) != (n_out,):
            raise ValueError("s must be [n_out, Cin] and count [n_out]")
        b.s, b.count = s.data_ptr(), count.data_ptr()
        if need_kernel:
            gw = torch.empty(cin, cout, dtype=torch.float32, device=dev)
            b.grad_kernel = gw.data_ptr()
        if need_bias:
            gb = torch.empty(cout, dtype=torch.float32, device=dev)
            b.grad_bias = gb.data_ptr()
    if gx is None and gw is None and gb is None:
        return None, None, None
    ws, nbytes = _workspace(dev, "dmcf_neighbor_dense_backward_workspace_bytes", ctypes.byref(b))
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_neighbor_dense_backward", ctypes.byref(b), _ptr(ws), nbytes, _stream())
    if timer is not None:
        timer.end("neighbor_dense_backward", dict(n_out=n_out, cin=int(cin), cout=int(cout),
                                                  kernel=neighbor_dense_kernel_names(None, b)), t0)
    del keep
    return gx, gw, gb


class NeighborDenseFunction(torch.autograd.Function):
    """Autograd node of :func:`neighbor_dense`: the same forward kernel, recording S and c; the backward is
    dmcf_neighbor_dense_backward (the list inverted on first need, or shared through ``kw['inverted']``).  The residual's
    gradient is grad_out itself."""

    @staticmethod
    def forward(ctx, x, kernel, bias, residual, kw):
        out, s, c = _nd_forward(x, kernel, bias, kw["neighbors_index"], kw["neighbors_row_splits"], kw["n_in"], kw["relu"],
                                residual, kw["neighbors_row_count"], record=True)
        ctx.kw = kw
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, kernel, s, c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, kernel, s, c = ctx.saved_tensors
        kw = ctx.kw
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        gx, gw, gb = neighbor_dense_backward(x.detach(), kernel.detach(), grad_out.contiguous(), s, c, n_in=kw["n_in"],
                                             relu=kw["relu"], inverted=kw["inverted"], neighbors_index=kw["neighbors_index"],
                                             neighbors_row_splits=kw["neighbors_row_splits"],
                                             neighbors_row_count=kw["neighbors_row_count"], need_x=need_x, need_kernel=need_w,
                                             need_bias=need_b and ctx.has_bias)
        return gx, gw, gb, (grad_out if need_r else None), None


def neighbor_dense(x, kernel, bias, neighbors_index, neighbors_row_splits, n_in=None, relu=True, residual=None,
                   neighbors_row_count=None, inverted=None):
    """PointNet's layer (models/pointnet.py:137-145 of the reference) in one launch (dmcf_neighbor_dense_forward):
    ``out[r] = sum_{p in row r} (act(x[idx[p]]) @ kernel + bias)`` (+ ``residual[r]``), act = relu or the identity.

    ``n_in``: the rows of ``x`` the indices may address (default: all of them).  A pair whose index is outside [0, n_in)
    contributes nothing, neither features nor bias -- what TensorFlow's GPU gather does for the reference's layer 0, which
    gathers fluid-only rows with indices over fluid and boundary points.  ``neighbors_row_count``: int32 [n_out] for padded
    lists.  When autograd records and an operand requires grad the call goes through :class:`NeighborDenseFunction`
    (``inverted``: an optional :class:`SharedInverse` of the list for the input gradient); otherwise it is the inference
    path: the same kernel, the same bits, no ``grad_fn``."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, kernel, bias, residual)):
        kw = dict(neighbors_index=neighbors_index, neighbors_row_splits=neighbors_row_splits, n_in=n_in, relu=bool(relu),
                  neighbors_row_count=neighbors_row_count, inverted=inverted)
        return NeighborDenseFunction.apply(x, kernel, bias, residual, kw)
    with torch.no_grad():
        return _nd_forward(x, kernel, bias, neighbors_index, neighbors_row_splits, n_in, relu, residual, neighbors_row_count)


class ScatterPlan:
    """dmcf_cconv_scatter_plan's output (include/dmcf_hip.h): the input points counting-sorted by the block of ``block_cells``^3
    lattice cells they lie in.  Depends on the two point sets, the lattice spacing and the radius only -- one plan serves every
    layer of a step between the same two sets.  Built on the device without a host round trip."""

    def __init__(self, buf, voxel, block_cells, reach, n_inp, keep):
        self.buf, self.voxel, self.block_cells, self.reach, self.n_inp = buf, float(voxel), int(block_cells), int(reach), int(n_inp)
        self._keep = keep  # (the operands the plan was made from)


SCATTER_BLOCK_CELLS = 4  # m: blocks of m^3 lattice cells (0.4 units of the 0.1 lattice of Liquid3d: ~500 particles)


@functools.lru_cache()
def _scatter_reach(extent, voxel):
    return int(_lib.lib().dmcf_cconv_scatter_reach(extent, voxel))


def scatter_reach(radius, voxel):
    """dmcf_cconv_scatter_reach for the extent scatter_plan passes: the lattice cells a radius covers, as the plan counts them."""
    return _scatter_reach(2.0 * float(radius), float(voxel))


def scatter_plan(inp_positions, out_positions, voxel, radius, block_cells=None):
    L = _lib.lib()
    inp = _dev_f32(inp_positions, "inp_positions", 3)
    out = _dev_f32(out_positions, "out_positions", 3)
    m = int(block_cells or SCATTER_BLOCK_CELLS)
    n = inp.shape[0]
    if n == 0 or out.shape[0] == 0:
        # (nothing to sort, and the C ABI rejects NULL point arrays: cconv_scatter_forward returns the bias for such a call
        # without reading the plan)
        return ScatterPlan(torch.empty(0, dtype=torch.uint8, device=inp.device), voxel, m, scatter_reach(radius, voxel), n, (inp, out))
    nbytes = L.dmcf_cconv_scatter_plan_bytes(n)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=inp.device)
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_cconv_scatter_plan", _ptr(inp), n, _ptr(out), out.shape[0], float(voxel), 2.0 * float(radius), m, _ptr(buf),
              nbytes, _stream())
    if timer is not None:
        timer.end("scatter_plan", dict(n_points=n), t0)
    return ScatterPlan(buf, voxel, m, scatter_reach(radius, voxel), n, (inp, out))


@functools.lru_cache()
def _scatter_pick(dims, block_cells, reach):
    """(status, name) of dmcf_cconv_scatter_kernel_name for a filter shape and a box."""
    name = ctypes.create_string_buffer(64)
    rc = _lib.lib().dmcf_cconv_scatter_kernel_name((ctypes.c_int32 * 5)(*dims), block_cells, reach, name, len(name))
    return rc, name.value.decode()


def scatter_kernel_name(cout, block_cells, reach):
    """The instantiation dmcf_cconv_scatter_forward launches, as rocprofv3 prints it (DmcfError for a box the library refuses)."""
    rc, name = _scatter_pick((4, 4, 4, 1, int(cout)), int(block_cells), int(reach))
    _lib.check(rc, "dmcf_cconv_scatter_kernel_name")
    return name


def cconv_scatter_supported(filters, block_cells, reach):
    """Does dmcf_cconv_scatter_forward take a layer of this filter shape with this box?"""
    return len(filters.shape) == 5 and _scatter_pick(tuple(int(d) for d in filters.shape), int(block_cells), int(reach))[0] == 0


def scatter_block_cells(cout, reach, most=SCATTER_BLOCK_CELLS):
    """The largest block_cells <= ``most`` whose box the library takes at this reach; 0: none."""
    return next((m for m in range(int(most), 0, -1) if _scatter_pick((4, 4, 4, 1, int(cout)), m, int(reach))[0] == 0), 0)


def _dev_exact_1d(t, name, dtype, device, length=None):
    """A 1-D operand the library reads through a raw pointer: ValueError unless it is a contiguous ``dtype`` tensor on ``device``
    (of ``length`` elements)."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1:
        raise ValueError(f"{name} must be a 1-D {dtype} tensor, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the filters on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if length is not None and t.shape[0] != length:
        raise ValueError(f"{name} must have {length} elements, got {t.shape[0]}")
    return t


def _scatter_operands(what, filters, out_positions, inp_positions, inp_features, t_index, t_row_begin, t_row_count, window):
    """The operand checks dmcf_cconv_scatter_forward and dmcf_cconv_scatter_backward share (ValueError / NotImplementedError
    before anything is launched); returns (filters, out_positions, inp_positions, inp_features) as the library reads them."""
    filters = _dev_f32(filters, "filters")
    if filters.dim() != 5:
        raise ValueError("filters must have shape [D,H,W,Cin,Cout]")
    out_positions = _dev_f32(out_positions, "out_positions", 3)
    inp_positions = _dev_f32(inp_positions, "inp_positions", 3)
    inp_features = _dev_f32(inp_features, "inp_features", int(filters.shape[3]))
    n_inp = inp_positions.shape[0]
    if window not in (None, "poly6"):
        raise NotImplementedError(f"{what}: window must be None or 'poly6'")
    dev = filters.device
    _dev_exact_1d(t_index, "t_index", torch.int32, dev)
    _dev_exact_1d(t_row_begin, "t_row_begin", torch.int64, dev)
    if t_row_count is not None:
        _dev_exact_1d(t_row_count, "t_row_count", torch.int32, dev)
    if inp_features.shape[0] != n_inp:
        raise ValueError("inp_features and inp_positions disagree on the number of points")
    if t_row_begin.shape[0] < n_inp + (1 if t_row_count is None else 0):
        raise ValueError("t_row_begin has fewer entries than the input points have rows")
    if t_row_count is not None and t_row_count.shape[0] < n_inp:
        raise ValueError("t_row_count has fewer entries than the input points have rows")
    return filters, out_positions, inp_positions, inp_features


def cconv_scatter_forward(filters, out_positions, extent, inp_positions, inp_features, t_index, t_row_begin, t_row_count, plan,
                          window=None, window_fac=1.0, bias=None, out=None, accumulate=False, error_flag=None, n_pairs_ref=None):
    """One call of dmcf_cconv_scatter_forward (splat S: filter first, input stationary, 64-bit fixed-point sums): the operator
    of cconv_forward for particles -> coarse lattice layers with 4 or 8 output channels, walking the TRANSPOSED list (row j = the
    output points within extent / 2 of input point j; ``t_row_count`` None for CSR row splits).  ``t_index`` int32,
    ``t_row_begin`` int64, ``t_row_count`` int32, ``bias`` float32 [Cout], ``error_flag`` int32: contiguous and on the filters'
    device (ValueError otherwise, before anything is launched).  An empty point set or an empty ``t_index`` gives the bias
    (prior content + bias under ``accumulate``) without a launch, as cconv_forward does.

    When autograd records (``torch.is_grad_enabled()``) and ``filters``, ``inp_features`` or ``bias`` requires grad, the call
    goes through ``ScatterConvFunction``: the same forward kernel, and a backward through dmcf_cconv_scatter_backward on the same
    transposed list.  ``bias`` is differentiable there (torch adds it after the kernel: its gradient is the column sum of the
    output's).  Every operand is checked as in a plain call, before the node is made.  ``out=`` / ``accumulate=True`` raise
    ValueError there.  Otherwise the call is exactly the inference path."""
    recording = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (filters, inp_features, bias))
    checked = _scatter_operands("cconv_scatter_forward", filters, out_positions, inp_positions, inp_features, t_index, t_row_begin,
                                t_row_count, window)
    cin, cout = int(checked[0].shape[3]), int(checked[0].shape[4])
    n_out, n_inp = checked[1].shape[0], checked[2].shape[0]
    if plan.n_inp != n_inp:
        raise ValueError("the plan was made for another input point set")
    reach = scatter_reach(float(extent) / 2, plan.voxel)
    if plan.reach != reach:
        raise ValueError(f"the plan was made for a reach of {plan.reach} lattice cells; extent {float(extent)} over its voxel "
                         f"{plan.voxel} has a reach of {reach}: make a plan for this radius (scatter_plan)")
    if not cconv_scatter_supported(checked[0], plan.block_cells, plan.reach):
        raise ValueError(f"the plan's block_cells {plan.block_cells} and reach {plan.reach} give a box the scatter form does not "
                         f"take for filters {tuple(checked[0].shape)} (scatter_block_cells)")
    dev = checked[0].device
    if bias is not None:
        _dev_exact_1d(bias, "bias", torch.float32, dev, cout)
    if error_flag is not None:
        _dev_exact_1d(error_flag, "error_flag", torch.int32, dev)
        if error_flag.shape[0] < 1:
            raise ValueError("error_flag must have at least one element")
    if recording:
        if out is not None or accumulate:
            raise ValueError("out= / accumulate=True cannot be recorded by autograd: use the returned tensor")
        # (the node takes the caller's own tensors, so that the graph reaches them; the call inside it checks them again)
        geo = dict(extent=float(extent), window=window, window_fac=window_fac)

        def run(w, f, **lists):
            return cconv_scatter_forward(w, inp_features=f, plan=plan, error_flag=error_flag, n_pairs_ref=n_pairs_ref, **lists, **geo)
        res = ScatterConvFunction.apply(filters, inp_features, out_positions, inp_positions, t_index, t_row_begin, t_row_count, geo, run)
        return res if bias is None else res + bias
    filters, out_positions, inp_positions, inp_features = checked
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs an out tensor")
        out = torch.empty((n_out, cout), dtype=torch.float32, device=filters.device)
    elif out.shape != (n_out, cout) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out has the wrong shape / dtype / layout / device")
    if n_out == 0 or n_inp == 0 or t_index.shape[0] == 0:
        # every row is empty: the result is the bias; nothing to launch (the C ABI rejects empty sets, and the kernel clamps its
        # index loads to the last entry of a list that has none)
        b = 0.0 if bias is None else bias
        if accumulate:
            out += b
        else:
            out[:] = b
        return out
    if plan.buf.numel() == 0:
        raise ValueError("the plan was made for an empty point set: make one for these points (scatter_plan)")
    a = _scatter_args(filters, out_positions, extent, inp_positions, inp_features, t_index, t_row_begin, t_row_count, window, window_fac,
                      plan=plan, bias=bias, out=out, error_flag=error_flag, flags=FLAG_ACCUMULATE if accumulate else 0)
    ws, nbytes = _workspace(filters.device, "dmcf_cconv_scatter_workspace_bytes", ctypes.byref(a), least=0)
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_cconv_scatter_forward", ctypes.byref(a), _ptr(ws), nbytes, _stream())
    if timer is not None:
        pairs = n_pairs_ref if n_pairs_ref is not None else (t_row_count.sum() if t_row_count is not None else t_row_begin[-1])
        timer.end("cconv", dict(pairs=pairs, n_out=n_out, cin=cin, cout=cout, K=64, symmetric=False,
                                kernel=scatter_kernel_name(cout, plan.block_cells, plan.reach), pair_values=False, accumulate=bool(accumulate)), t0)
    return out


def _scatter_args(filters, out_positions, extent, inp_positions, inp_features, t_index, t_row_begin, t_row_count, window, window_fac,
                  plan=None, bias=None, out=None, error_flag=None, flags=0):
    """struct dmcf_cconv_scatter_args of a forward call, or of the backward's (which reads no plan, bias, out or error flag)."""
    a = _lib.CconvScatterArgs()
    a.filters = _ptr(filters)
    for k in range(5):
        a.filter_dims[k] = int(filters.shape[k])
    a.out_positions, a.n_out = _ptr(out_positions), out_positions.shape[0]
    a.inp_positions, a.n_inp = _ptr(inp_positions), inp_positions.shape[0]
    a.inp_features = _ptr(inp_features)
    a.t_index, a.t_row_begin = _ptr(t_index), _ptr(t_row_begin)
    a.t_row_count = _ptr(t_row_count) if t_row_count is not None else None
    a.t_capacity = int(t_index.shape[0])
    if plan is not None:
        a.plan, a.block_cells, a.reach = _ptr(plan.buf), plan.block_cells, plan.reach
    a.extent, a.window_fac, a.window = float(extent), float(window_fac), WINDOWS[window]
    a.flags = FLAG_ALIGN_CORNERS | flags
    a.bias = _ptr(bias) if bias is not None else None
    a.out = _ptr(out) if out is not None else None
    a.error_flag = _ptr(error_flag) if error_flag is not None else None
    return a


def cconv_scatter_backward(filters, out_positions, extent, inp_positions, inp_features, t_index, t_row_begin, t_row_count, grad_out,
                           window=None, window_fac=1.0, need_filters=True, need_features=True):
    """dmcf_cconv_scatter_backward: ``(grad_filters | None, grad_inp_features | None)`` of the convolution
    :func:`cconv_scatter_forward` computes with these arguments (bias excluded), for ``grad_out`` = dL/d out [n_out, Cout].  One
    walk over the TRANSPOSED list (row j = the output points within extent / 2 of input point j; ``t_row_count`` None for CSR
    row splits) gives both: no plan, no list inversion, no float atomics (two calls return the same bits).  Operands as
    cconv_scatter_forward takes them, checked as strictly.  Rows of ``grad_inp_features`` of input points without pairs are
    zero.  Empty point sets or an empty ``t_index`` give zero gradients without a launch."""
    filters, out_positions, inp_positions, inp_features = _scatter_operands(
        "cconv_scatter_backward", filters, out_positions, inp_positions, inp_features, t_index, t_row_begin, t_row_count, window)
    cin, cout = int(filters.shape[3]), int(filters.shape[4])
    n_out, n_inp = out_positions.shape[0], inp_positions.shape[0]
    dev = filters.device
    grad_out = _dev_f32(grad_out, "grad_out", cout)
    if grad_out.shape[0] != n_out or grad_out.device != dev:
        raise ValueError("grad_out must be [n_out, Cout] on the filters' device")
    if not need_filters and not need_features:
        return None, None
    if n_out == 0 or n_inp == 0 or t_index.shape[0] == 0:
        # every row is empty: no pair, no gradient; nothing to launch (the C ABI rejects empty sets)
        return (torch.zeros_like(filters) if need_filters else None,
                torch.zeros((n_inp, cin), dtype=torch.float32, device=dev) if need_features else None)
    gw = torch.empty(tuple(filters.shape), dtype=torch.float32, device=dev) if need_filters else None
    gf = torch.empty((n_inp, cin), dtype=torch.float32, device=dev) if need_features else None
    a = _scatter_args(filters, out_positions, extent, inp_positions, inp_features, t_index, t_row_begin, t_row_count, window, window_fac)
    b = _lib.CconvScatterBackwardArgs()
    b.struct_size = ctypes.sizeof(_lib.CconvScatterBackwardArgs)
    b.flags = 0
    b.grad_out = _ptr(grad_out)
    b.grad_filters = _ptr(gw) if need_filters else None
    b.grad_inp_features = _ptr(gf) if need_features else None
    ws, nbytes = _workspace(dev, "dmcf_cconv_scatter_backward_workspace_bytes", ctypes.byref(a), ctypes.byref(b), least=0)
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_cconv_scatter_backward", ctypes.byref(a), ctypes.byref(b), _ptr(ws), nbytes, _stream())
    if timer is not None:
        timer.end("cconv_backward", dict(n_out=n_out, n_inp=n_inp, cin=cin, cout=cout, filters=bool(need_filters),
                                         features=bool(need_features), kernel="cconv_sct_bwd"), t0)
    return gw, gf


class ScatterConvFunction(torch.autograd.Function):
    """Autograd node of the input-stationary CConv: ``run(filters, inp_features, out_positions=, inp_positions=, t_index=,
    t_row_begin=, t_row_count=)`` is the forward (cconv_scatter_forward, or any kernel that computes the same operator on the same
    pairs; bias excluded: torch adds it), the backward is one dmcf_cconv_scatter_backward over the same transposed list with the
    options in ``geo`` (extent, window, window_fac).  The node saves the filters, the features, both position tensors and the list
    themselves -- the per-step cache forgets them when the step ends --, so a tensor changed in place between forward and
    backward is an error, not another gradient.  Positions get no gradient; the backward is not differentiable again."""

    @staticmethod
    def forward(ctx, filters, inp_features, out_positions, inp_positions, t_index, t_row_begin, t_row_count, geo, run):
        ctx.geo = geo
        ctx.save_for_backward(filters, inp_features, out_positions, inp_positions, t_index, t_row_begin, t_row_count)
        # (grad mode is off in here, so this is the plain call)
        return run(filters, inp_features, out_positions=out_positions, inp_positions=inp_positions, t_index=t_index,
                   t_row_begin=t_row_begin, t_row_count=t_row_count)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        filters, inp_features, out_positions, inp_positions, t_index, t_row_begin, t_row_count = ctx.saved_tensors
        need_w, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gw = gf = None
        if need_w or need_f:
            gw, gf = cconv_scatter_backward(filters, out_positions, ctx.geo["extent"], inp_positions, inp_features, t_index,
                                            t_row_begin, t_row_count, grad_out.contiguous(), window=ctx.geo["window"],
                                            window_fac=ctx.geo["window_fac"], need_filters=need_w, need_features=need_f)
        return gw, gf, None, None, None, None, None, None, None


def continuous_conv(filters, out_positions, extents, offset, inp_positions, inp_features, inp_importance,
                    neighbors_index, neighbors_row_splits, neighbors_importance, align_corners=True,
                    coordinate_mapping="ball_to_cube_radial", interpolation="linear", normalize=True,
                    max_temp_mem_MB=64, **_ignored):
    """Mirror of ``ml3d.ops.continuous_conv`` with the keyword set of utils/convolutions.py:414-431.

    ``extents``: a single value (every shipped DMCF config, :352-353,:390-392) or individual extents of shape [n_out] or
    [n_out, 1] (the RadiusSearch branch, :366-370 and :397-399); anisotropic extents ([n_out, 3], [1, 3]) are not implemented.
    ``offset`` must be zero (:200-201).  An empty tensor means "absent" for the importance inputs (:335,:376).
    """
    ext = extents if isinstance(extents, torch.Tensor) else torch.as_tensor(extents)
    if ext.dim() == 2 and ext.shape[1] == 3:
        raise NotImplementedError("anisotropic extents ([n, 3] / [1, 3]) are not used by DMCF and not implemented")
    if offset is not None and bool(torch.as_tensor(offset).ne(0).any()):
        raise NotImplementedError("non-zero offset is not used by DMCF and not implemented")
    window = None if _empty(neighbors_importance) else "explicit"
    return cconv_forward(filters, out_positions, float(ext) if ext.numel() == 1 else ext, inp_positions, inp_features, neighbors_index,
                         neighbors_row_splits, neighbors_value=neighbors_importance, window=window,
                         inp_importance=inp_importance, align_corners=align_corners,
                         coordinate_mapping=coordinate_mapping, interpolation=interpolation, normalize=normalize)


SPARSE_NEGATE, SPARSE_W_TRANSPOSED, SPARSE_ACCUMULATE = 1, 2, 4  # DMCF_SPARSE_*


def _sparse_offset(offset):
    o = [0.0, 0.0, 0.0] if offset is None else [float(v) for v in torch.as_tensor(offset).reshape(-1).tolist()]
    if len(o) != 3:
        raise ValueError("offset must have shape [3]")
    return o


def _sparse_vec(t, name, n, device):
    """An optional per-point scale: None / empty -> None, else a float32 [n] device tensor."""
    if _empty(t):
        return None
    t = _dev_f32(t, name)
    if t.dim() != 1 or t.shape[0] != n or t.device != device:
        raise ValueError(f"{name} must be a float32 [{n}] tensor on {device}")
    return t


def _sparse_bias(bias, channels, device):
    """None, or a float32 [channels] tensor on ``device`` (DmcfError for a CPU tensor, as for every operand of the hot path)."""
    if bias is None:
        return None
    bias = _dev_f32(bias, "bias")
    if bias.dim() != 1 or bias.shape[0] != channels or bias.device != device:
        raise ValueError(f"bias must be a float32 [{channels}] tensor on {device}, got {tuple(bias.shape)} on {bias.device}")
    return bias


def _sparse_args(filters, row_positions, col_positions, col_features, index, row_splits, extent, offset, flags, row_scale=None,
                 col_scale=None, bias=None, out=None):
    """struct dmcf_sparse_conv_args for the row-gather operator of include/dmcf_hip.h, and the tensors it points to."""
    filters = _dev_f32(filters, "filters")
    if filters.dim() != 5:
        raise ValueError("filters must have shape [kz, ky, kx, Cin, Cout]")
    dev = filters.device
    bias = _sparse_bias(bias, filters.shape[3] if flags & SPARSE_W_TRANSPOSED else filters.shape[4], dev)
    row_positions = _dev_f32(row_positions, "row positions", 3)
    col_positions = _dev_f32(col_positions, "col positions", 3)
    xc = filters.shape[4] if flags & SPARSE_W_TRANSPOSED else filters.shape[3]
    col_features = _dev_f32(col_features, "features", xc)
    n_rows, n_cols = row_positions.shape[0], col_positions.shape[0]
    if col_features.shape[0] != n_cols:
        raise ValueError("one feature row per column point")
    if index.dtype != torch.int32 or row_splits.dtype != torch.int64 or not index.is_cuda or not row_splits.is_cuda:
        raise TypeError("neighbors_index must be int32 and neighbors_row_splits int64, both on the GPU")
    if row_splits.shape[0] != n_rows + 1:
        raise ValueError("neighbors_row_splits must have n_rows + 1 entries")
    index, row_splits = index.contiguous(), row_splits.contiguous()
    row_scale = _sparse_vec(row_scale, "row scale", n_rows, dev)
    col_scale = _sparse_vec(col_scale, "col scale", n_cols, dev)
    a = _lib.SparseConvArgs()
    a.struct_size = ctypes.sizeof(_lib.SparseConvArgs)
    a.flags = flags
    a.filters = filters.data_ptr()
    for k in range(5):
        a.filter_dims[k] = filters.shape[k]
    a.row_positions, a.n_rows = row_positions.data_ptr(), n_rows
    a.col_positions, a.n_cols = col_positions.data_ptr(), n_cols
    a.col_features = col_features.data_ptr()
    a.row_scale = None if row_scale is None else row_scale.data_ptr()
    a.col_scale = None if col_scale is None else col_scale.data_ptr()
    a.neighbors_index = index.data_ptr()
    a.neighbors_row_splits = row_splits.data_ptr()
    a.n_pairs = index.shape[0]
    a.extent = float(extent)
    for k in range(3):
        a.offset[k] = offset[k]
    a.bias = None if bias is None else bias.data_ptr()
    a.out = None if out is None else out.data_ptr()
    keep = (filters, row_positions, col_positions, col_features, index, row_splits, row_scale, col_scale, bias, out)
    return a, keep, dev


def sparse_conv_kernel_names(a, backward=0):
    """';'-separated kernels dmcf_sparse_conv_forward (``backward`` 0) / _backward (1: filters, 2: features, 3: both) launches."""
    return _kernel_name("dmcf_sparse_conv_kernel_names", ctypes.byref(a), int(backward), size=128).decode()


def sparse_gather(filters, row_positions, col_positions, col_features, index, row_splits, extent, offset, flags=0, row_scale=None,
                  col_scale=None, bias=None, out=None):
    """dmcf_sparse_conv_forward: ``out[r] = row_scale[r] * sum_p col_scale[j] * W[cell(+-(col_pos[j] - row_pos[r]))]^T x[j] (+ bias)``
    over the CSR list (index, row_splits); see include/dmcf_hip.h.  No list, no rows or no columns: the bias-only result,
    without a launch."""
    offset = _sparse_offset(offset)
    a, keep, dev = _sparse_args(filters, row_positions, col_positions, col_features, index, row_splits, extent, offset, flags,
                                row_scale, col_scale, bias, None)
    oc = filters.shape[3] if flags & SPARSE_W_TRANSPOSED else filters.shape[4]
    if out is None:
        if flags & SPARSE_ACCUMULATE:
            raise ValueError("SPARSE_ACCUMULATE adds into ``out``: pass the tensor to add into")
        out = torch.empty((a.n_rows, oc), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (a.n_rows, oc) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous float32 [{a.n_rows}, {oc}] tensor on {dev}")
    if a.n_rows == 0 or a.n_cols == 0 or a.n_pairs == 0:
        if not flags & SPARSE_ACCUMULATE:
            out.zero_()
        if keep[8] is not None:
            out += keep[8]
        return out
    a.out = out.data_ptr()
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_sparse_conv_forward", ctypes.byref(a), _stream())
    if timer is not None:
        timer.end("sparse_conv", dict(n_rows=int(a.n_rows), cin=int(filters.shape[3]), cout=int(filters.shape[4])), t0)
    del keep
    return out


def sparse_gather_backward(filters, row_positions, col_positions, col_features, index, row_splits, extent, offset, grad_out, flags=0,
                           row_scale=None, col_scale=None, need_filters=True, need_features=True, inverted=None):
    """dmcf_sparse_conv_backward: ``(grad_filters, grad_col_features)`` of :func:`sparse_gather` with these arguments.
    ``inverted``: an ``invert_neighbors_list(n_cols, index, row_splits)`` result (formed here when the feature gradient is
    wanted and none is given)."""
    offset = _sparse_offset(offset)
    a, keep, dev = _sparse_args(filters, row_positions, col_positions, col_features, index, row_splits, extent, offset,
                                flags & ~SPARSE_ACCUMULATE, row_scale, col_scale)
    oc = filters.shape[3] if flags & SPARSE_W_TRANSPOSED else filters.shape[4]
    grad_out = _dev_f32(grad_out, "grad_out", oc)
    if grad_out.shape[0] != a.n_rows:
        raise ValueError("grad_out must have one row per output row")
    gw = gf = None
    if need_filters:
        gw = torch.empty(tuple(filters.shape), dtype=torch.float32, device=dev)
    if need_features:
        gf = torch.empty(tuple(col_features.shape), dtype=torch.float32, device=dev)
    if a.n_rows == 0 or a.n_cols == 0 or a.n_pairs == 0:
        return (None if gw is None else gw.zero_()), (None if gf is None else gf.zero_())
    if not need_filters and not need_features:
        return None, None
    inv_index = inv_rs = None
    inv_pairs = 0
    if need_features:
        if inverted is None:
            inverted = invert_neighbors_list(a.n_cols, keep[4], keep[5])
        inv_index, inv_rs = inverted.neighbors_index, inverted.neighbors_row_splits
        inv_pairs = inv_index.shape[0]
    ws, nbytes = _workspace(dev, "dmcf_sparse_conv_backward_workspace_bytes", ctypes.byref(a), 1 if need_filters else 0, least=16)
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_sparse_conv_backward", ctypes.byref(a), _ptr(grad_out), _ptr(inv_index), _ptr(inv_rs), inv_pairs, _ptr(gw),
              _ptr(gf), _ptr(ws), nbytes, _stream())
    if timer is not None:
        timer.end("sparse_conv_backward", dict(n_rows=int(a.n_rows), filters=bool(need_filters), features=bool(need_features)), t0)
    del keep
    return gw, gf


class SparseGatherFunction(torch.autograd.Function):
    """Autograd node of :func:`sparse_gather` (bias excluded: torch adds it): the backward is dmcf_sparse_conv_backward, the list
    inverted once when the features want a gradient.  Positions and scales get no gradient here (a scale that wants one is
    applied by torch outside the node, see sparse_conv)."""

    @staticmethod
    def forward(ctx, filters, col_features, geo):
        ctx.geo = geo
        ctx.save_for_backward(filters, col_features)
        return sparse_gather(filters, col_features=col_features, **geo)

    @staticmethod
    def backward(ctx, grad_out):
        filters, col_features = ctx.saved_tensors
        need_w, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not need_w and not need_f:
            return None, None, None
        gw, gf = sparse_gather_backward(filters.detach(), col_features=col_features.detach(), grad_out=grad_out.contiguous(),
                                        need_filters=need_w, need_features=need_f, **ctx.geo)
        return gw, gf, None


def _sparse_call(filters, features, bias, row_scale, col_scale, geo):
    """The fused call, or -- when something wants a gradient -- the autograd node with torch around it for what the node does
    not differentiate: a scale that requires grad is applied outside, the bias is added outside."""
    wants = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (filters, features, bias, row_scale, col_scale))
    bias = _sparse_bias(bias, filters.shape[3] if geo["flags"] & SPARSE_W_TRANSPOSED else filters.shape[4], filters.device)
    if not wants:
        return sparse_gather(filters, col_features=features, bias=bias, row_scale=row_scale, col_scale=col_scale, **geo)
    if col_scale is not None and col_scale.requires_grad:
        features, col_scale = features * col_scale[:, None], None
    outer = None
    if row_scale is not None and row_scale.requires_grad:
        outer, row_scale = row_scale, None
    geo = dict(geo, row_scale=None if row_scale is None else row_scale.detach(), col_scale=None if col_scale is None else col_scale.detach())
    out = SparseGatherFunction.apply(filters, features, geo)
    if outer is not None:
        out = out * outer[:, None]
    return out if bias is None else out + bias


def _row_count_scale(row_splits):
    """1 / |row| per row of a CSR list, 0 for an empty row (float32, on the device)."""
    cnt = torch.diff(row_splits).to(torch.float32)
    return torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt))


def sparse_conv(filters, out_positions, voxel_size, offset, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
                inp_importance=None, normalize=False, bias=None):
    """What ``SparseConv`` asks of ``ml3d.ops.continuous_conv`` (utils/convolutions.py:645-664: identity mapping, align_corners
    False, nearest neighbour, extent = voxel_size * kernel_size[-1]) on the voxel-convolution kernel:
    ``out_i = s_i sum_j imp_j W[cell(inp_j - out_i)]^T f_j (+ bias)`` over the list's row i, ``s_i = 1 / |row i|`` with
    ``normalize`` (0 for an empty row).  ``filters`` [kz, ky, kx, Cin, Cout]; ``offset`` [3] in cells.  Differentiable in
    filters, features, bias and importance."""
    filters = _dev_f32(filters, "filters")
    n_out, n_inp = out_positions.shape[0], inp_positions.shape[0]
    dev = filters.device
    imp = _sparse_vec(inp_importance, "inp_importance", n_inp, dev)
    rs = _row_count_scale(neighbors_row_splits) if normalize else None
    geo = dict(row_positions=out_positions, col_positions=inp_positions, index=neighbors_index, row_splits=neighbors_row_splits,
               extent=float(np.float32(voxel_size) * np.float32(filters.shape[2])), offset=_sparse_offset(offset), flags=0)
    return _sparse_call(filters, inp_features, bias, rs, imp, geo)


def sparse_conv_transpose(filters, out_positions, voxel_size, offset, inp_positions, inp_features, inp_neighbors_index,
                          inp_neighbors_row_splits, neighbors_index, neighbors_row_splits, out_importance=None, normalize=False,
                          bias=None):
    """What ``SparseConvTranspose`` asks of ``ml3d.ops.continuous_conv_transpose`` (utils/convolutions.py:852-874):
    ``out_i = oimp_i sum_{j in row i} n_j W[cell(out_i - inp_j)]^T f_j (+ bias)`` over the INVERTED list (neighbors_index,
    neighbors_row_splits: for every output point the input points whose search found it); ``n_j = 1 / |N_T(j)|`` with
    ``normalize``, from the input points' list (inp_neighbors_row_splits).  The direction of the relative position (output
    minus input) is this project's reading of Open3D's operator."""
    filters = _dev_f32(filters, "filters")
    n_out, n_inp = out_positions.shape[0], inp_positions.shape[0]
    dev = filters.device
    oimp = _sparse_vec(out_importance, "out_importance", n_out, dev)
    if inp_neighbors_row_splits.shape[0] != n_inp + 1:
        raise ValueError("inp_neighbors_row_splits must have n_inp + 1 entries")
    cs = _row_count_scale(inp_neighbors_row_splits) if normalize else None
    geo = dict(row_positions=out_positions, col_positions=inp_positions, index=neighbors_index, row_splits=neighbors_row_splits,
               extent=float(np.float32(voxel_size) * np.float32(filters.shape[2])), offset=_sparse_offset(offset), flags=SPARSE_NEGATE)
    return _sparse_call(filters, inp_features, bias, oimp, cs, geo)


def dense_supported(x, kernel):
    """Does :func:`dense_forward` take this product (else the caller keeps torch's GEMM)?"""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and x.shape[1] % 4 == 0
            and 0 < x.shape[1] <= 64 and 0 < kernel.shape[1] <= 64 and x.data_ptr() % 16 == 0)


def dense_forward(x, kernel, bias=None, residual=None):
    """``x @ kernel (+ bias) (+ residual)``: the networks' Dense layers on a million rows (dmcf_dense_forward)."""
    n, k = x.shape
    m = kernel.shape[1]
    kernel = _dev_f32(kernel, "kernel")
    out = torch.empty(n, m, dtype=torch.float32, device=x.device)
    if residual is not None:
        residual = _dev_f32(residual, "residual")
        if tuple(residual.shape) != (n, m):
            raise ValueError("residual must be [n, m]")
    _lib.call("dmcf_dense_forward", _ptr(x), n, k, _ptr(kernel), m, _ptr(bias) if bias is not None else None,
              _ptr(residual) if residual is not None else None, _ptr(out), _stream())
    return out


def points_aabb(points, row_splits=None):
    """(min, max) over axis 0 of [n, 3] float32 points, two [3] device tensors: the fluid bounds of the boundary crop
    (models/pbf_model.py:330-336) in two small launches (a torch reduction over the strided columns was 0.2 ms + a transpose).

    ``row_splits`` (a sequence, a CPU or a device int64 tensor): the bounds of every item of a batch in one launch
    (dmcf_points_aabb_batched) -> two [batch, 3] tensors; an item's bounds are those of the call on its slice, except that an
    empty item gives +3.0e38 / -3.0e38 (the model's box of "no fluid") where the un-batched call gives +inf / -inf."""
    if row_splits is not None:
        host, dev = _host_row_splits(row_splits, "row_splits")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be [n, 3]")
        _check_row_splits(host, points.shape[0], "row_splits")
        points = _dev_f32(points, "points")
        batch = len(host) - 1
        out = torch.empty((batch, 6), dtype=torch.float32, device=points.device)
        _lib.call("dmcf_points_aabb_batched", _ptr(points), points.shape[0], _ptr(_row_splits_on(host, dev, points.device)), batch,
                  _ptr(out), _stream())
        return out[:, :3], out[:, 3:]
    L = _lib.lib()
    points = _dev_f32(points, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be [n, 3]")
    out = torch.empty(6, dtype=torch.float32, device=points.device)
    wsb = int(L.dmcf_points_aabb_workspace_bytes())
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=points.device)
    _lib.call("dmcf_points_aabb", _ptr(points), points.shape[0], _ptr(out), _ptr(ws), wsb, _stream())
    return out[:3], out[3:]


def reduce_subarrays_sum(values, row_splits):
    """Mirror of ``o3dml.ops.reduce_subarrays_sum`` (models/pbf_model.py:450-453)."""
    values = _dev_f32(values, "values")
    if row_splits.dtype != torch.int64:
        raise TypeError("row_splits must be int64")
    n_rows = row_splits.shape[0] - 1
    out = torch.empty(n_rows, dtype=torch.float32, device=values.device)
    _lib.call("dmcf_reduce_subarrays_sum", _ptr(values), _ptr(row_splits.contiguous()), n_rows, _ptr(out), _stream())
    return out


def neighbor_counts(row_splits):
    """``reduce_subarrays_sum(ones_like(neighbors_index), row_splits)`` without materialising the ones
    (models/pbf_model.py:450-453): float32 neighbour count per row.  Also accepts a search result."""
    if isinstance(row_splits, PaddedNeighborList):
        return row_splits.row_count.to(torch.float32)
    if isinstance(row_splits, NeighborSearchResult):
        row_splits = row_splits.neighbors_row_splits
    if row_splits.dtype != torch.int64 or not row_splits.is_cuda:
        raise _lib.DmcfError("row_splits must be an int64 GPU tensor")
    n_rows = row_splits.shape[0] - 1
    out = torch.empty(n_rows, dtype=torch.float32, device=row_splits.device)
    _lib.call("dmcf_reduce_subarrays_sum", None, _ptr(row_splits.contiguous()), n_rows, _ptr(out), _stream())
    return out


GRID_MAX_CELLS = 1 << 31  # dense cell table of the lattice bounding box: 4 bytes per cell, at most 8 GiB ...
# ... and at most this many cells per particle (+ a floor): a few particles that left the scene (a splash; a particle falling
# forever) stretch the bounding box, and a table that grows with it is a fresh multi-GB hipMalloc in every step of the
# rollout (measured on the 100k-particle dam break: 6 -> 8 GB per step until the 8 GiB cap).  Beyond it: the sort-based form.
GRID_MAX_CELLS_PER_POINT = 64
GRID_MIN_CELLS = 1 << 22


_GRID_CELLS = {}  # (voxel sizes of the levels, flags) -> cells of each level's box at the last call: grid_pos_many's estimates


class GridTooSparse(RuntimeError):
    """The bounding box of the candidate cells has more than GRID_MAX_CELLS cells (a few particles very far apart):
    the caller uses the sort-based device formulation instead."""


def _grid_too_sparse(cells, n):
    """Too sparse for the dense cell table (a few particles far from the rest): the hashed table (include/dmcf_hip.h)."""
    return cells > min(GRID_MAX_CELLS, max(GRID_MIN_CELLS, GRID_MAX_CELLS_PER_POINT * n))


def _grid_hash_slots(n, voxel, pad):
    """Slots of the hashed table: a power of two of at least twice the 2 n n_off candidates."""
    import numpy as np
    noff = 1
    for x in np.asarray(voxel, dtype=np.float32).reshape(3):
        noff *= (2 + 2 * int(pad)) if x >= 1e-5 else 1
    return 1 << max(int(4 * n * noff - 1).bit_length(), 10)


def _grid_cell_table(capacity, device):
    if capacity < 0:  # hashed: 4 + 8 bytes per slot
        return torch.empty(3 * (-capacity), dtype=torch.int32, device=device)
    return torch.empty(max(capacity, 1), dtype=torch.int32, device=device)


def _grid_count_levels(levels, key, count, read_headers, hash_slots):
    """The count passes of all levels of one grid_pos_many call, with or without row splits, and their host round trips.
    ``count(lv, capacity)`` enqueues a level's count pass on a table of ``capacity`` cells (< 0: hashed slots);
    ``read_headers()`` brings every level's "cells", "sparse" and totals to the host.

    A rollout asks for the same levels step after step and their boxes move slowly: with the cell count of the last call as an
    estimate (+ 1/4, in size classes) the count pass runs BEFORE anything is read, and ONE host round trip brings header and point
    count of every level; a level whose box outgrew its table is counted again with the exact size (a second round trip, rare)."""
    est = _GRID_CELLS.get(key)
    if est is not None and len(est) == len(levels):
        for lv, c in zip(levels, est):  # (c < 0: the level was sparse at the last call)
            count(lv, -hash_slots if c < 0 else _size_class(c + c // 4))
        read_headers()
        again = [lv for lv in levels if lv["capacity"] >= 0 and (lv["sparse"] or lv["cells"] > lv["capacity"])]
        for lv in again:
            count(lv, -hash_slots if lv["sparse"] else lv["cells"])
        if again:
            read_headers()
    else:
        read_headers()  # (host round trip 1 of 2: every level's header)
        for lv in levels:
            count(lv, -hash_slots if lv["sparse"] else lv["cells"])
        read_headers()  # (host round trip 2 of 2: every level's point count)
    while len(_GRID_CELLS) > 32:  # (virtual ranks are threads sharing this dict: evict without iterating a dict another thread resizes)
        try:
            _GRID_CELLS.pop(next(iter(_GRID_CELLS)), None)
        except (RuntimeError, StopIteration):
            break
    _GRID_CELLS[key] = [-1 if lv["sparse"] else lv["cells"] for lv in levels]


class RowSplits:
    """Row splits in both forms: ``host`` a tuple of batch + 1 ints, ``dev`` the same as an int64 device tensor.  Every
    ``row_splits`` argument takes one, and then copies nothing to validate it.  A batched ``grid_pos`` returns its output row
    splits as one (``dev``: what the count pass wrote; ``sparse``: whether the call took the hashed cell table)."""

    def __init__(self, host, dev, sparse=False):
        self.host, self.dev, self.sparse = tuple(host), dev, sparse


def grid_pos_many(pos, voxel_sizes, centralize=False, pad=0, hyst=0.1, center=None, row_splits=None):
    """``grid_pos`` (utils/tools/losses.py:136-181) for SEVERAL voxel sizes over the same positions -- the coarse levels of one step
    (losses.py:266-272) -- via dmcf_grid_pos_bounds/_count/_write with TWO host round trips for all of them (cells of every level,
    then points of every level) instead of two per level.  -> [(points, (minp, dims) | None), ...].  A level whose box is too sparse
    for the dense cell table (GRID_MAX_CELLS_PER_POINT) takes the hashed table; GridTooSparse is no longer raised (round 6).

    ``row_splits`` (a sequence, a CPU or a device int64 tensor): ``pos`` is a BATCH of point sets, item b = pos[rs[b]:rs[b+1]]
    (dmcf_grid_pos_*_batched) -> [(points, RowSplits), ...]: every level's points are the concatenation, item after item, of
    what the un-batched call returns for each slice, bit for bit; ``center``, if given, is [batch, 3].  The same two round trips
    bring every item's header (its cells), then every item's point count, which IS the output row splits.  These lattices are
    not registered with dmcf_amd/lattice.py: the lattice and scatter forms of ContinuousConv know nothing of items."""
    import numpy as np
    batched = row_splits is not None
    if batched:
        host, dev = _host_row_splits(row_splits, "row_splits")  # (every host-side check before a device is touched)
        if pos.dim() != 2 or pos.shape[1] != 3:
            raise ValueError("pos must be [n, 3]")
        _check_row_splits(host, pos.shape[0], "row_splits")
        batch = len(host) - 1
        if center is not None and tuple(center.shape) != (batch, 3):
            raise ValueError(f"center must be [batch, 3] = [{batch}, 3] with row_splits, got {tuple(center.shape)}")
    L = _lib.lib()
    pos = _dev_f32(pos, "pos", 3)
    n = pos.shape[0]
    cflag = 1 if centralize else 0
    # the entry points of the call and what the batched ones take after (positions, n): the un-batched ones take no row splits
    if batched:
        bounds_fn, count_fn, write_fn = "dmcf_grid_pos_bounds_batched", "dmcf_grid_pos_count_batched", "dmcf_grid_pos_write_batched"
        rs = _row_splits_on(host, dev, pos.device)
        items = (_ptr(rs), batch)
        cen = _dev_f32(center, "center") if center is not None else None
        ws_bytes = L.dmcf_grid_pos_workspace_bytes_batched(n, batch)
        if ws_bytes == 0:
            raise _lib.DmcfError(f"grid_pos: a batch of {batch} items is not supported")
    else:
        bounds_fn, count_fn, write_fn = "dmcf_grid_pos_bounds", "dmcf_grid_pos_count", "dmcf_grid_pos_write"
        items, batch = (), 1
        cen = _dev_f32(center.reshape(3), "center") if center is not None else None
        ws_bytes = L.dmcf_grid_pos_workspace_bytes(n)
    levels = []
    for v in voxel_sizes:
        vs = (ctypes.c_float * 3)(*[float(x) for x in np.asarray(v, dtype=np.float32).reshape(3)])
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
        _lib.call(bounds_fn, _ptr(pos), n, *items, vs, cflag, _ptr(cen) if cen is not None else None, int(pad), float(hyst),
                  _ptr(ws), ws_bytes, _stream())
        # (ors: the output row splits, the batched count pass's extra argument)
        levels.append(dict(vs=vs, ws=ws, ors=torch.empty(batch + 1, dtype=torch.int64, device=pos.device) if batched else None))

    def read_headers():
        hdrs = torch.stack([lv["ws"][0:64 * batch] for lv in levels]).cpu()
        for lv, hdr in zip(levels, hdrs):
            words = hdr.view(torch.int64).reshape(batch, 8)
            cells, lv["totals"] = words[:, 3].tolist(), words[:, 4].tolist()
            if any(c < 0 for c in cells):
                raise _lib.DmcfError("grid_pos: positions are not finite")
            lv["cells"] = sum(cells)  # the dense table holds every item's own box, one after the other
            if not batched:
                lv["center_host"] = hdr[40:52].view(torch.float32).tolist()
                lv["minp"], lv["dims"] = hdr[0:12].view(torch.int32).tolist(), hdr[12:24].view(torch.int32).tolist()
            # too sparse for the dense cell table (a few particles far from the rest): the hashed table (include/dmcf_hip.h).
            # The rule is applied to the call: all cells against all points
            lv["sparse"] = _grid_too_sparse(lv["cells"], n)

    def count(lv, capacity):
        lv["table"], lv["capacity"] = _grid_cell_table(capacity, pos.device), capacity
        _lib.call(count_fn, _ptr(pos), n, *items, lv["vs"], cflag, int(pad), float(hyst), _ptr(lv["ws"]), ws_bytes,
                  _ptr(lv["table"]), capacity, *([_ptr(lv["ors"])] if batched else []), _stream())

    # (the estimates are keyed with the batch size: a training loop asks for the same batch step after step)
    key = (tuple(tuple(float(x) for x in lv["vs"]) for lv in levels), bool(centralize), int(pad), float(hyst))
    if batched:
        key += (batch,)
    _grid_count_levels(levels, key, count, read_headers, max(_grid_hash_slots(n, v, pad) for v in voxel_sizes))
    res = []
    for lv in levels:
        total = sum(lv["totals"])
        out = torch.empty((total, 3), dtype=torch.float32, device=pos.device)
        if total:
            _lib.call(write_fn, _ptr(pos), n, *items, lv["vs"], cflag, int(pad), float(hyst), _ptr(lv["ws"]), ws_bytes,
                      _ptr(lv["table"]), lv["capacity"], _ptr(out), total, _stream())
        if batched:
            out_host = [0]
            for t in lv["totals"]:
                out_host.append(out_host[-1] + t)
            res.append((out, RowSplits(tuple(out_host), lv["ors"], lv["capacity"] < 0)))
            continue
        if total and centralize and center is None:
            # out = float(cell) * voxel + mean(pos): every lattice built from these positions shares the centre exactly
            # (dmcf_amd/lattice.py; the lattice form of ContinuousConv uses it)
            from . import lattice
            # (the entry keeps ``pos`` alive: its address + version identify the family for as long as the entry exists)
            lattice.register(out, lv["ws"][40:52].view(torch.float32).clone(), [float(v) for v in lv["vs"]],
                             ("mean", pos.data_ptr(), pos.shape[0], pos._version), lv["minp"], lv["dims"], keep=pos,
                             center_host=lv["center_host"])
        res.append((out, (lv["minp"], lv["dims"]) if total else None))
    return res


def grid_pos(pos, voxel_size, centralize=False, pad=0, hyst=0.1, center=None, return_box=False, row_splits=None):
    """Lattice points of ``grid_pos`` (utils/tools/losses.py:136-181) via dmcf_grid_pos_bounds/_count/_write.
    ``voxel_size``: 3 host floats; ``center``: optional [3] GPU tensor (lattice origin instead of the mean).
    ``return_box``: -> (points, (minp, dims) | None): the integer box of cells of THIS call (None for an empty result).
    ``row_splits``: a batch of point sets (see grid_pos_many) -> (points, RowSplits); ``center`` is then [batch, 3]."""
    if row_splits is not None:
        if return_box:
            raise NotImplementedError("grid_pos: return_box with row_splits (a batch has one box per item)")
        return grid_pos_many(pos, [voxel_size], centralize, pad, hyst, center, row_splits=row_splits)[0]
    out, box = grid_pos_many(pos, [voxel_size], centralize, pad, hyst, center)[0]
    return (out, box) if return_box else out


class GhostSelection:
    """A started ghost selection (dmcf_ghost_count has run): ``totals`` int64 [W, B] on the device = entries box b contributes to
    the list of width w.  :meth:`write` produces the lists once their sizes are known on the host."""

    def __init__(self, pos, boxes, widths2, ws, totals):
        self.pos, self.boxes, self.widths2, self.ws, self.totals = pos, boxes, widths2, ws, totals

    def write(self, sizes):
        """``sizes``: entries of list(w) per width (host ints: the row sums of ``totals``, read by the caller -- or known from the
        ranks that counted the same points).  -> [int64 tensor of list(w) for every w]: box-major, ascending point index."""
        W, B = self.totals.shape
        sizes = [int(v) for v in sizes]
        starts = [0]
        for v in sizes[:-1]:
            starts.append(starts[-1] + v)
        rows = torch.empty(max(sum(sizes), 1), dtype=torch.int64, device=self.pos.device)
        c64 = ctypes.c_int64 * W
        w2 = (ctypes.c_float * W)(*self.widths2)
        _lib.call("dmcf_ghost_write", _ptr(self.pos), self.pos.shape[0], _ptr(self.boxes), B, w2, W, _ptr(rows), c64(*starts),
                  c64(*sizes), _ptr(self.ws), self.ws.numel(), _stream())
        return [rows[starts[w]: starts[w] + sizes[w]] for w in range(W)]


def ghost_select(pos, boxes, widths2):
    """dmcf_ghost_count: for every point of ``pos`` [n, 3] and every box of ``boxes`` [B, 6] (lo xyz, hi xyz; device float32) the
    number of ``widths2`` (host floats, DESCENDING) its squared distance to the box does not exceed.  ``widths2`` = [-1.0] selects
    OWNERSHIP instead (lo <= x < hi per axis): one list, the stable order of the points by owning box.  Returns a
    :class:`GhostSelection`."""
    pos = _dev_f32(pos, "pos", 3)
    boxes = _dev_f32(boxes.reshape(-1, 6), "boxes", 6)
    B, W = boxes.shape[0], len(widths2)
    widths2 = [float(np.float32(v)) for v in widths2]
    ws, nbytes = _workspace(pos.device, "dmcf_ghost_workspace_bytes", pos.shape[0], B, W, least=0)
    totals = torch.empty((W, B), dtype=torch.int64, device=pos.device)
    w2 = (ctypes.c_float * W)(*widths2)
    _lib.call("dmcf_ghost_count", _ptr(pos), pos.shape[0], _ptr(boxes), B, w2, W, _ptr(totals), _ptr(ws), nbytes, _stream())
    return GhostSelection(pos, boxes, widths2, ws, totals)


def _window_sum_impl(points, queries, radius, window, flags, hash_table, batched=None):
    """dmcf_frs_window_sum, or with ``batched`` (WindowSumFunction's triple) dmcf_frs_window_sum_batched, under the span
    frs_window_sum_batched -> (out, item_max or None, the search structure over ``points`` that served the call, the queries'
    device splits or None)."""
    n, m = points.shape[0], queries.shape[0]
    dev = points.device
    p_splits, (q_host, q_dev), want_max = batched if batched is not None else (None, (None, None), False)
    batch = None if batched is None else len(q_host) - 1
    hash_table = _serving_table(hash_table, points, radius, m, p_splits)
    nbytes = _frs_workspace_bytes(n, hash_table.n_queries_capacity, batch)
    out = torch.empty(m, dtype=torch.float32, device=dev)
    q_rs = item_max = None
    if batched is None:
        entry, item, tail = "dmcf_frs_window_sum", (), ()
    else:
        q_rs = _row_splits_on(q_host, q_dev, dev)
        item_max = torch.empty(batch, dtype=torch.float32, device=dev) if want_max else None
        entry, item, tail = "dmcf_frs_window_sum_batched", (_ptr(q_rs), batch), (_ptr(item_max),)
    t0 = timer.begin() if timer is not None and batched is not None else None
    _lib.call(entry, _ptr(queries), m, *item, n, radius, flags, WINDOWS[window], _ptr(hash_table.workspace), nbytes, _ptr(out), *tail,
              _stream())
    if t0 is not None:
        timer.end("frs_window_sum_batched", dict(n_points=n, n_queries=m, batch=batch), t0)
    return out, item_max, hash_table, q_rs


def window_sum_backward(queries, hash_table, radius, window, coef_queries=None, coef_points=None, ignore_query_point=False,
                        queries_row_splits=None):
    """dmcf_frs_window_sum_backward on the structure ``hash_table`` of some point set: float32 [m, 3],
    ``grad[q] = 2 sum_{|p - q| <= R} (coef_queries[q] + coef_points[p]) dw/d(d^2) (q - p)``.  ``coef_queries`` [m] and
    ``coef_points`` [n points of the structure] may each be None (0), not both.  Distance set only (DMCF_FRS_SET=distance).

    ``queries_row_splits`` (as for the batched search, with as many items as the structure): on the batched structure of some
    concatenated point sets (dmcf_frs_window_sum_backward_batched), the sums of a query running over the points of its own
    item.  A batched structure needs them, the structure of a single point set takes none (ValueError either way)."""
    batched = queries_row_splits is not None
    if batched and hash_table.row_splits is None:
        raise ValueError("hash_table is not a batched structure (build_spatial_hash_table(..., points_row_splits=...))")
    if not batched and hash_table.row_splits is not None:
        raise ValueError("hash_table is a batched structure: pass queries_row_splits")
    if batched:
        q_host, q_dev = _host_row_splits(queries_row_splits, "queries_row_splits")
        _check_row_splits(q_host, queries.shape[0], "queries_row_splits")
        if len(q_host) != len(hash_table.row_splits):
            raise ValueError("queries_row_splits and the structure's row splits must have equal lengths (batch + 1)")
    queries = _dev_f32(queries, "queries", 3)
    radius = float(radius)
    if window not in WINDOWS:
        raise NotImplementedError(f"window {window!r}")
    n, m = hash_table.points.shape[0], queries.shape[0]
    if hash_table.n_queries_capacity < m or hash_table.radius != radius:
        raise ValueError("hash_table was built for fewer queries or another radius")
    dev = queries.device
    cq = None if coef_queries is None else _dev_exact(coef_queries, "coef_queries", torch.float32, (m,), dev)
    cp = None if coef_points is None else _dev_exact(coef_points, "coef_points", torch.float32, (n,), dev)
    if batched:
        q_rs = _row_splits_on(q_host, q_dev, dev)
        batch = len(q_host) - 1
        entry, item = "dmcf_frs_window_sum_backward_batched", (_ptr(q_rs), batch)
    else:
        batch = None
        entry, item = "dmcf_frs_window_sum_backward", ()
    nbytes = _frs_workspace_bytes(n, hash_table.n_queries_capacity, batch)
    grad = torch.empty((m, 3), dtype=torch.float32, device=dev)
    _lib.call(entry, _ptr(queries), m, *item, n, radius, frs_flags(ignore_query_point, batched), WINDOWS[window], _ptr(cq), _ptr(cp),
              _ptr(hash_table.workspace), nbytes, _ptr(grad), _stream())
    return grad


def _window_sum_backward_pairs(points, queries, radius, window, ignore_query_point, grad_out, need_points, need_queries):
    """The gradient of ``window_sum`` on the explicit pair list with torch ops: the form for the open3d readings of the search
    (DMCF_FRS_SET=open3d / open3d_corners), whose pair set is not symmetric -- swapping the roles of the two sets would scan other
    pairs than the forward summed.  Correct but slow (a [P]-sized gather and scatter per operand)."""
    from .utils.tools.losses import WindowFunction
    nns = fixed_radius_search(points, queries, radius, ignore_query_point=ignore_query_point, return_distances=False)
    idx, rs = nns.neighbors_index.long(), nns.neighbors_row_splits
    m = queries.shape[0]
    row = torch.repeat_interleave(torch.arange(m, device=queries.device), torch.diff(rs), output_size=idx.shape[0])
    with torch.enable_grad():
        p = points.detach().requires_grad_(need_points)
        q = queries.detach().requires_grad_(need_queries)
        d2 = ((p[idx] - q[row]) ** 2).sum(-1)
        if window == "explicit":
            w = d2
        else:
            keep = d2.detach() > 0 if window != "poly6" else None  # (a coincident pair of a sqrt-based window contributes 0)
            if keep is not None:
                d2, row = d2[keep], row[keep]
            w = WindowFunction(window)(d2 / (radius * radius))
        out = torch.zeros(m, dtype=torch.float32, device=queries.device).index_add(0, row, w)
        wanted = [t for t, need in ((p, need_points), (q, need_queries)) if need]
        grads = list(torch.autograd.grad(out, wanted, grad_out))
    gp = grads.pop(0) if need_points else None
    gq = grads.pop(0) if need_queries else None
    return gp, gq


class WindowSumFunction(torch.autograd.Function):
    """Autograd node of ``window_sum``: the gradient w.r.t. both position sets through dmcf_frs_window_sum_backward -- the
    forward's structure serves the query side, one built over the queries the point side; ``same``: the two sets are one tensor
    and one scan with both coefficients gives the whole gradient (returned for ``points``).

    ``batched`` (None, or ((points splits), (queries splits), return_item_max) with each splits a (host, dev) pair): the same
    on batched structures (dmcf_frs_window_sum_batched / dmcf_frs_window_sum_backward_batched); the point side then takes a
    batched structure over the queries with the roles of the two row splits swapped.  With return_item_max the node returns
    (out, item_max), item_max non-differentiable."""

    @staticmethod
    def forward(ctx, points, queries, radius, window, ignore_query_point, hash_table, same, batched=None):
        ctx.batched = batched
        flags = frs_flags(ignore_query_point, batched is not None)
        out, item_max, table, ctx.q_rs = _window_sum_impl(points, queries, radius, window, flags, hash_table, batched)
        if window is None:
            ctx.mark_non_differentiable(out)  # (the count)
        ctx.save_for_backward(points, queries)
        ctx.radius, ctx.window, ctx.ignore, ctx.table, ctx.same, ctx.flags = radius, window, ignore_query_point, table, same, flags
        if item_max is not None:
            ctx.mark_non_differentiable(item_max)
            return out, item_max
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, *_grad_item_max):
        points, queries = ctx.saved_tensors
        need_p, need_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        rest = (None,) * 6
        if ctx.window is None or not (need_p or need_q):
            return (None, None) + rest
        g = grad_out.contiguous()
        n, m = points.shape[0], queries.shape[0]
        p_splits = q_splits = None
        if ctx.batched is not None:
            (p_host, _), (q_host, _), _ = ctx.batched
            p_splits, q_splits = RowSplits(p_host, ctx.table.row_splits_dev), RowSplits(q_host, ctx.q_rs)
        elif frs_flags(ctx.ignore) != ctx.flags:
            raise RuntimeError("DMCF_FRS_SET changed between the forward and the backward of window_sum")
        if n == 0 or m == 0:  # no pair
            return (torch.zeros_like(points) if need_p else None, torch.zeros_like(queries) if need_q else None) + rest
        if ctx.batched is None and search_set() != "distance":
            gp, gq = _window_sum_backward_pairs(points, queries, ctx.radius, ctx.window, ctx.ignore, g, need_p, need_q)
            if ctx.same:
                gp, gq = gp + gq, None
            return (gp, gq) + rest
        if ctx.same:
            return (window_sum_backward(queries, ctx.table, ctx.radius, ctx.window, g, g, ctx.ignore, q_splits), None) + rest
        gp = gq = None
        if need_q:
            gq = window_sum_backward(queries, ctx.table, ctx.radius, ctx.window, g, None, ctx.ignore, q_splits)
        if need_p:  # (the roles swapped: a structure over the queries, with their row splits)
            swapped = build_spatial_hash_table(queries, ctx.radius, n_queries=n, points_row_splits=q_splits)
            gp = window_sum_backward(points, swapped, ctx.radius, ctx.window, None, g, ctx.ignore, p_splits)
        return (gp, gq) + rest


def window_sum(points, queries, radius, window=None, ignore_query_point=False, hash_table=None, points_row_splits=None,
               queries_row_splits=None, return_item_max=False):
    """dmcf_frs_window_sum: out[q] = sum_{|p - q| <= R} window(|p - q|^2 / R^2) (``window``: a WINDOWS key; None counts
    the neighbours, 'explicit' sums the squared distances).  The fused form of ``compute_density``
    (utils/tools/losses.py:285-306): the candidate scan of the search with the sum inside, no pair list.

    Differentiable in ``points`` and ``queries`` (dmcf_frs_window_sum_backward: the same scan with three sums; the count,
    ``window=None``, is marked non-differentiable).  For the sqrt-based windows a coincident pair contributes no gradient, where
    the reference's autodiff gives NaN.  Under DMCF_FRS_SET=open3d / open3d_corners the backward takes the explicit pair list and
    torch ops instead: correct, but slow.  Without grad mode or an input that requires grad the call is the plain kernel launch.

    ``points_row_splits`` / ``queries_row_splits`` (both or neither; the rules of the batched ``fixed_radius_search``): the sums
    of a BATCH of point sets in one call (dmcf_frs_window_sum_batched), a query summing over the points of its own item only.
    A batched ``hash_table`` built with the same splits is reused (as everywhere, a table that does not serve the call -- other
    points, radius or splits, too few queries, a batched one without row splits -- is replaced by a new one).
    ``return_item_max=True`` returns ``(out, item_max)`` with
    ``item_max`` [batch] each item's largest sum (0 for an item without queries; not differentiable; not with 'cubic_grad',
    whose sums can be negative).  It needs row splits: pass ``[0, n]`` and ``[0, m]`` for one item."""
    batched = None
    same = points is queries
    if points_row_splits is not None or queries_row_splits is not None:
        # host checks first, in the order of the batched search: both or neither, no walk emulation, well-formed splits
        if points_row_splits is None or queries_row_splits is None:
            raise NotImplementedError("batched window_sum needs both points_row_splits and queries_row_splits")
        if SEARCH_SETS[search_set()] != 0:
            raise NotImplementedError(f"DMCF_FRS_SET={search_set()} has no batched form: the open3d walk emulations know nothing of items")
        if window not in WINDOWS:
            raise NotImplementedError(f"window {window!r}")
        p_splits, q_splits = _batched_row_splits(points, queries, points_row_splits, queries_row_splits)
        if same and p_splits[0] != q_splits[0]:
            raise ValueError("points is queries, but points_row_splits and queries_row_splits differ")
        batched = (p_splits, q_splits, bool(return_item_max))
    elif return_item_max:
        raise NotImplementedError("return_item_max needs points_row_splits and queries_row_splits")
    points = _dev_f32(points, "points", 3)
    queries = points if same else _dev_f32(queries, "queries", 3)
    radius = float(radius)
    if batched is not None and not radius > 0:
        raise ValueError("radius must be positive")
    if window not in WINDOWS:
        raise NotImplementedError(f"window {window!r}")
    if _wants_grad(points, queries):
        return WindowSumFunction.apply(points, queries, radius, window, bool(ignore_query_point), hash_table, same, batched)
    flags = frs_flags(ignore_query_point, batched is not None)
    out, item_max = _window_sum_impl(points, queries, radius, window, flags, hash_table, batched)[:2]
    return (out, item_max) if return_item_max else out


def farthest_point_sample(npoint, inp):
    """Mirror of ``utils/tools/sampling.py: farthest_point_sample(npoint, inp)``: ``inp`` [1, n, 3] -> int32 [1, npoint]
    (dmcf_farthest_point_sample; the batch dimension of this path is always 1, utils/tools/losses.py:278-279)."""
    if inp.dim() != 3 or inp.shape[0] != 1 or inp.shape[2] != 3:
        raise ValueError("farthest_point_sample expects a [1, n, 3] tensor")
    pts = _dev_f32(inp[0], "inp", 3)
    n, m = pts.shape[0], int(npoint)
    if m > 0 and n == 0:
        raise ValueError("cannot sample from an empty point set")
    ws, nbytes = _workspace(pts.device, "dmcf_fps_workspace_bytes", n, least=0)
    idx = torch.empty(m, dtype=torch.int32, device=pts.device)
    _lib.call("dmcf_farthest_point_sample", _ptr(pts), n, m, _ptr(ws), nbytes, _ptr(idx), _stream())
    return idx.unsqueeze(0)


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _dev_exact(t, name, dtype, shape, device):
    """The operand ``t`` of a backward entry point: a tensor of ``dtype`` and exactly ``shape`` on ``device`` (a GPU), made
    contiguous; anything else raises before a pointer reaches the library."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if not t.is_cuda:
        raise _lib.DmcfError(f"{name} is on {t.device}: the DMCF hot path runs on the GPU only (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the point sets on {device}")
    return t.contiguous()


def _sets3(xyz1, xyz2):
    """Both point sets of a backward entry point: float32 GPU tensors of shape exactly [b, n, 3] / [b, m, 3] (the padded batches
    the forward works on), same b and device -> contiguous (xyz1, xyz2)."""
    a, _ = _point_batch(xyz1, "xyz1")
    b, _ = _point_batch(xyz2, "xyz2")
    for t, name in ((xyz1, "xyz1"), (xyz2, "xyz2")):
        if t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError(f"{name} must have shape [b, n, 3] here, got {tuple(t.shape)}")
    if a.shape[0] != b.shape[0] or a.device != b.device:
        raise ValueError(f"xyz1 {tuple(xyz1.shape)} and xyz2 {tuple(xyz2.shape)} must have the same batch size and device")
    return a, b


def _gather_point_impl(x, ii):
    out = torch.empty((ii.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    _lib.call("dmcf_gather_point", _ptr(x), _ptr(ii), ii.shape[0], x.shape[1], _ptr(out), _stream())
    return out


def gather_point_backward(grad_out, idx, n_inp):
    """dmcf_gather_point_backward: grad_inp [n_inp, c] = sum of the rows of ``grad_out`` [m, c] whose ``idx`` [m] (int32) points
    at the row; repeated indices sum, in ascending order of m (no atomics)."""
    g = _dev_f32(grad_out, "grad_out")
    if g.dim() != 2 or g.shape[1] == 0:
        raise ValueError(f"grad_out must have shape [m, c] with c > 0, got {tuple(g.shape)}")
    m, c = g.shape
    idx = _dev_exact(idx, "idx", torch.int32, (m,), g.device)
    n_inp = int(n_inp)
    if n_inp < 0:
        raise ValueError(f"n_inp must be >= 0, got {n_inp}")
    grad_inp = torch.empty((n_inp, c), dtype=torch.float32, device=g.device)
    ws, nbytes = _workspace(g.device, "dmcf_gather_point_backward_workspace_bytes", m, n_inp)
    _lib.call("dmcf_gather_point_backward", _ptr(g), _ptr(idx), m, c, int(n_inp), _ptr(grad_inp), _ptr(ws), nbytes, _stream())
    return grad_inp


class GatherPointFunction(torch.autograd.Function):
    """Autograd node of ``gather_point`` (GatherPointGrad, sampling.py:78-83): the index gets no gradient."""

    @staticmethod
    def forward(ctx, x, ii):
        ctx.save_for_backward(ii)
        ctx.n_inp = x.shape[0]
        return _gather_point_impl(x, ii)

    @staticmethod
    def backward(ctx, grad_out):
        (ii,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return gather_point_backward(grad_out.contiguous(), ii, ctx.n_inp), None


def gather_point(inp, idx):
    """Mirror of ``gather_point(inp [1, n, c], idx [1, m]) -> [1, m, c]`` (utils/tools/sampling.py).  Differentiable in
    ``inp`` (dmcf_gather_point_backward)."""
    if inp.dim() != 3 or inp.shape[0] != 1 or idx.dim() != 2 or idx.shape[0] != 1:
        raise ValueError("gather_point expects inp [1, n, c] and idx [1, m]")
    x = _dev_f32(inp[0], "inp")
    if idx.dtype != torch.int32 or not idx.is_cuda:
        raise TypeError("idx must be an int32 GPU tensor")
    ii = idx[0].contiguous()
    out = GatherPointFunction.apply(x, ii) if _wants_grad(x) else _gather_point_impl(x, ii)
    return out.unsqueeze(0)


# ---------------------------------------------------------------------------------------------------------------------
# validation metrics (pipelines/simulator.py:167-285): nn_distance (Chamfer), approx_match / match_cost / emd (EMD)
# ---------------------------------------------------------------------------------------------------------------------
def _point_batch(t, name):
    """[b, n, 2|3] or [n, 2|3] float32 GPU tensor -> contiguous [b, n, 3] (2-D scenes padded with z = 0), batched flag."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if not t.is_cuda:
        raise _lib.DmcfError(f"{name} is on {t.device}: the DMCF hot path runs on the GPU only (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    batched = t.dim() == 3
    if t.dim() not in (2, 3) or t.shape[-1] not in (2, 3):
        raise ValueError(f"{name} must have shape [b, n, 3], [b, n, 2], [n, 3] or [n, 2], got {tuple(t.shape)}")
    if not batched:
        t = t.unsqueeze(0)
    if t.shape[-1] == 2:
        t = torch.nn.functional.pad(t, (0, 1))
    return t.contiguous(), batched


def _pair_batch(xyz1, xyz2):
    a, b1 = _point_batch(xyz1, "xyz1")
    b, b2 = _point_batch(xyz2, "xyz2")
    if b1 != b2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"xyz1 {tuple(xyz1.shape)} and xyz2 {tuple(xyz2.shape)} must have the same batch size")
    if a.device != b.device:
        raise ValueError("xyz1 and xyz2 must be on the same device")
    return a, b, b1


def _host_counts(c, b, limit, name):
    """None | int | sequence | array | tensor of b point counts -> None or a host int32 array (dmcf_approx_match reads it on
    the host, before anything is enqueued)."""
    if c is None:
        return None
    if isinstance(c, torch.Tensor):
        c = c.detach().cpu().numpy()
    arr = np.asarray(c, dtype=np.int64).reshape(-1)
    if arr.size == 1 and b != 1:
        arr = np.full(b, int(arr[0]), dtype=np.int64)
    if arr.size != b:
        raise ValueError(f"{name} must hold one count per batch item ({b}), got {arr.size}")
    if (arr < 0).any() or (arr > limit).any():
        raise ValueError(f"{name} must lie in [0, {limit}], got {arr.tolist()}")
    return np.ascontiguousarray(arr, dtype=np.int32)


def _counts_ptr(arr):
    return None if arr is None else arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _nn_distance_impl(a, b):
    nb, n, m = a.shape[0], a.shape[1], b.shape[1]
    dev = a.device
    d1 = torch.empty((nb, n), dtype=torch.float32, device=dev)
    i1 = torch.empty((nb, n), dtype=torch.int32, device=dev)
    d2 = torch.empty((nb, m), dtype=torch.float32, device=dev)
    i2 = torch.empty((nb, m), dtype=torch.int32, device=dev)
    if nb > 0:
        ws, nbytes = _workspace(dev, "dmcf_nn_distance_workspace_bytes", nb, n, m)
        _lib.call("dmcf_nn_distance", _ptr(a), _ptr(b), nb, n, m, _ptr(d1), _ptr(i1), _ptr(d2), _ptr(i2), _ptr(ws), nbytes,
                  _stream())
    return d1, i1, d2, i2


def nn_distance_backward(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2, need1=True, need2=True):
    """dmcf_nn_distance_backward on [b, n, 3] / [b, m, 3] point sets and the forward's int32 indices: (grad_xyz1, grad_xyz2)
    (None where not wanted).  ``grad_dist1`` / ``grad_dist2`` None: zero.  No atomics: the scattered terms are gathered through a
    sort of the index list."""
    xyz1, xyz2 = _sets3(xyz1, xyz2)
    nb, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if nb > 0 and (n == 0 or m == 0):
        raise ValueError("nn_distance needs two non-empty point sets")
    dev = xyz1.device
    g1 = None if grad_dist1 is None else _dev_exact(grad_dist1, "grad_dist1", torch.float32, (nb, n), dev)
    g2 = None if grad_dist2 is None else _dev_exact(grad_dist2, "grad_dist2", torch.float32, (nb, m), dev)
    idx1 = None if g1 is None else _dev_exact(idx1, "idx1", torch.int32, (nb, n), dev)
    idx2 = None if g2 is None else _dev_exact(idx2, "idx2", torch.int32, (nb, m), dev)
    gx1 = torch.empty((nb, n, 3), dtype=torch.float32, device=dev) if need1 else None
    gx2 = torch.empty((nb, m, 3), dtype=torch.float32, device=dev) if need2 else None
    if nb > 0 and (need1 or need2):
        ws, nbytes = _workspace(dev, "dmcf_nn_distance_backward_workspace_bytes", nb, n, m)
        _lib.call("dmcf_nn_distance_backward", _ptr(xyz1), _ptr(xyz2), nb, n, m, _ptr(idx1), _ptr(idx2), _ptr(g1), _ptr(g2),
                  _ptr(gx1), _ptr(gx2), _ptr(ws), nbytes, _stream())
    return gx1, gx2


class NnDistanceFunction(torch.autograd.Function):
    """Autograd node of ``nn_distance`` (NnDistanceGrad, nn_distance.py:61-68): dist1 and dist2 are differentiable, the
    indices are not.  A distance output that takes no part in the loss arrives as None and counts as zero."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.set_materialize_grads(False)
        d1, i1, d2, i2 = _nn_distance_impl(a, b)
        ctx.mark_non_differentiable(i1, i2)
        ctx.save_for_backward(a, b, i1, i2)
        return d1, i1, d2, i2

    @staticmethod
    def backward(ctx, gd1, _gi1, gd2, _gi2):
        a, b, i1, i2 = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (gd1 is None and gd2 is None) or not (need1 or need2):
            return None, None
        return nn_distance_backward(a, b, i1, i2, gd1, gd2, need1, need2)


def nn_distance_row_splits(shape1, shape2, row_splits1, row_splits2, wants_grad=False, record=False):
    """The host-side checks of nn_distance with row splits on the shapes of the two point sets, all of them before a device is
    touched, in the order of the other batched ops: both or neither and no gradient (NotImplementedError), then well-formed
    splits, equal batch sizes and no item with exactly one empty set (ValueError).  ``record=True``: the caller records, so a
    wanted gradient is no refusal; everything else stays.  -> (host splits 1, host splits 2)."""
    if row_splits1 is None or row_splits2 is None:
        raise NotImplementedError("batched nn_distance needs both row_splits1 and row_splits2")
    for shape, name in ((shape1, "xyz1"), (shape2, "xyz2")):
        if len(shape) != 2 or shape[-1] not in (2, 3):
            raise ValueError(f"{name} must have shape [n_total, 3] or [n_total, 2] with row splits, got {tuple(shape)}")
    if wants_grad and not record:
        raise NotImplementedError("batched nn_distance has no backward unless it records (nn_distance_ragged(..., record=True)): "
                                  "call it under no_grad, or per item without row splits")
    s1 = _host_row_splits(row_splits1, "row_splits1")[0]
    s2 = _host_row_splits(row_splits2, "row_splits2")[0]
    _check_row_splits(s1, shape1[0], "row_splits1")
    _check_row_splits(s2, shape2[0], "row_splits2")
    if len(s1) != len(s2):
        raise ValueError(f"row_splits1 and row_splits2 must have equal lengths (batch + 1), got {len(s1)} and {len(s2)}")
    for k in range(len(s1) - 1):
        if (s1[k + 1] == s1[k]) != (s2[k + 1] == s2[k]):
            raise ValueError(f"nn_distance needs two non-empty point sets: item {k} has {s1[k + 1] - s1[k]} and "
                             f"{s2[k + 1] - s2[k]} points")
    return s1, s2


class NnDistanceRaggedFunction(torch.autograd.Function):
    """Autograd node of :func:`nn_distance_ragged` with ``record=True``.  The ragged forward's indices are rows of the
    concatenated sets, so the gradient is dmcf_nn_distance_backward on the [1, n_total, 3] / [1, m_total, 3] views: the
    inversion sorts the sources stably by target, an item's sources are contiguous and ascending, and a target's sum depends on
    the length of its segment alone -- every item's rows have the bits of the call on the item alone.  A distance output that
    takes no part in the loss (or was not wanted) arrives as None and counts as zero."""

    @staticmethod
    def forward(ctx, a, b, s1, s2, want1, want2):
        ctx.set_materialize_grads(False)
        d1, i1, d2, i2 = _nn_distance_ragged_impl(a, b, s1, s2, want1, want2)
        ctx.mark_non_differentiable(*(i for i in (i1, i2) if i is not None))
        ctx.save_for_backward(a, b, i1, i2)
        return d1, i1, d2, i2

    @staticmethod
    def backward(ctx, gd1, _gi1, gd2, _gi2):
        a, b, i1, i2 = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (gd1 is None and gd2 is None) or not (need1 or need2):
            return None, None, None, None, None, None
        if a.shape[1] == 0:  # (every item empty on both sides)
            return (torch.zeros_like(a) if need1 else None), (torch.zeros_like(b) if need2 else None), None, None, None, None
        gx1, gx2 = nn_distance_backward(a, b, None if i1 is None else i1.unsqueeze(0), None if i2 is None else i2.unsqueeze(0),
                                        None if gd1 is None else gd1.unsqueeze(0), None if gd2 is None else gd2.unsqueeze(0),
                                        need1, need2)
        return gx1, gx2, None, None, None, None


def nn_distance_ragged(xyz1, xyz2, row_splits1, row_splits2, want1=True, want2=True, record=False):
    """nn_distance with row splits (dmcf_nn_distance_ragged: one launch per wanted direction).  ``want1`` / ``want2``: a
    direction that is not wanted is not computed and returns (None, None).

    ``record=True``: differentiable.  When grad mode is on and an input requires grad, the wanted distances carry a grad_fn
    (:class:`NnDistanceRaggedFunction`; same bits as the call that does not record), and every item's gradient rows have the bits
    of the un-batched call on the item alone.  With ``record=False`` (the default) such inputs raise NotImplementedError."""
    for t, name in ((xyz1, "xyz1"), (xyz2, "xyz2")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
    wants_grad = _wants_grad(xyz1, xyz2)
    s1, s2 = nn_distance_row_splits(xyz1.shape, xyz2.shape, row_splits1, row_splits2, wants_grad, record=record)
    if not (want1 or want2):
        raise ValueError("nn_distance: no direction wanted")
    a, _ = _point_batch(xyz1, "xyz1")
    b, _ = _point_batch(xyz2, "xyz2")
    if a.device != b.device:
        raise ValueError("xyz1 and xyz2 must be on the same device")
    if record and wants_grad:
        return NnDistanceRaggedFunction.apply(a, b, s1, s2, want1, want2)
    return _nn_distance_ragged_impl(a, b, s1, s2, want1, want2)


def _nn_distance_ragged_impl(a, b, s1, s2, want1, want2):
    batch = len(s1) - 1
    n, m, dev = a.shape[1], b.shape[1], a.device
    d1 = torch.empty(n, dtype=torch.float32, device=dev) if want1 else None
    i1 = torch.empty(n, dtype=torch.int32, device=dev) if want1 else None
    d2 = torch.empty(m, dtype=torch.float32, device=dev) if want2 else None
    i2 = torch.empty(m, dtype=torch.int32, device=dev) if want2 else None
    if n > 0:
        ws, nbytes = _workspace(dev, "dmcf_nn_distance_ragged_workspace_bytes", n, m, batch)
        h1, h2 = (ctypes.c_int64 * (batch + 1))(*s1), (ctypes.c_int64 * (batch + 1))(*s2)
        _lib.call("dmcf_nn_distance_ragged", _ptr(a), n, h1, _ptr(b), m, h2, batch, _ptr(d1), _ptr(i1), _ptr(d2), _ptr(i2),
                  _ptr(ws), nbytes, _stream())
    return d1, i1, d2, i2


def nn_distance(xyz1, xyz2, row_splits1=None, row_splits2=None):
    """Mirror of ``utils/tools/nn_distance.py: nn_distance(xyz1, xyz2)`` -> ``(dist1, idx1, dist2, idx2)``: for each point of
    xyz1 [b, n, 3] the squared distance to its nearest point of xyz2 [b, m, 3] and that point's int32 index ([b, n]), and the
    same from xyz2 to xyz1 ([b, m]).  Equal distances go to the lowest index (dmcf_nn_distance).  dist1 and dist2 are
    differentiable in both point sets (dmcf_nn_distance_backward).

    ``row_splits1`` / ``row_splits2`` (both or neither; a sequence, a CPU or device int64 tensor or a :class:`RowSplits`): a
    RAGGED batch in one call (dmcf_nn_distance_ragged).  xyz1 is then [n_total, 3] and xyz2 [m_total, 3], item b being
    xyz1[rs1[b]:rs1[b + 1]] against xyz2[rs2[b]:rs2[b + 1]]; the results run over the concatenated rows ([n_total] and
    [m_total]) and equal the un-batched call on every item alone bit for bit, the indices offset by the item's first row of
    the other set.  An item with both sets empty is legal, one with exactly one empty set a ValueError.  No gradient here:
    inputs that require grad raise NotImplementedError.  :func:`nn_distance_ragged` computes one direction alone, and with
    ``record=True`` it is differentiable."""
    if row_splits1 is not None or row_splits2 is not None:
        return nn_distance_ragged(xyz1, xyz2, row_splits1, row_splits2)
    a, b, batched = _pair_batch(xyz1, xyz2)
    nb, n, m = a.shape[0], a.shape[1], b.shape[1]
    if nb > 0 and (n == 0 or m == 0):
        raise ValueError("nn_distance needs two non-empty point sets")
    out = NnDistanceFunction.apply(a, b) if _wants_grad(a, b) else _nn_distance_impl(a, b)
    return out if batched else tuple(x[0] for x in out)


def dense_match_fits(b, n, m, device=None):
    """True when a dense [b, m, n] float32 match fits in the free device memory (with a quarter to spare)."""
    need = 4 * int(b) * int(n) * int(m)
    free = torch.cuda.mem_get_info(device)[0]
    return need <= 0.75 * free


def approx_match(xyz1, xyz2, n=None, m=None):
    """Mirror of ``utils/tools/tf_approxmatch.py: approx_match(xyz1, xyz2, n, m)`` -> match [b, m, n] (dmcf_approx_match).
    ``n`` / ``m``: per-batch point counts (None: all points); rows and columns past a count are 0.  Refuses, before anything
    runs, a dense matrix that would not fit on the device: use :func:`emd` for the cost alone."""
    a, b, batched = _pair_batch(xyz1, xyz2)
    nb, nn_, mm = a.shape[0], a.shape[1], b.shape[1]
    c1, c2 = _host_counts(n, nb, nn_, "n"), _host_counts(m, nb, mm, "m")
    if not dense_match_fits(nb, nn_, mm, a.device):
        raise MemoryError(f"approx_match: the dense match [{nb}, {mm}, {nn_}] needs {4 * nb * nn_ * mm / 2 ** 30:.1f} GiB, more "
                          "than the device has free; ops.emd computes the matching cost without forming it")
    match = torch.empty((nb, mm, nn_), dtype=torch.float32, device=a.device)
    ws, nbytes = _workspace(a.device, "dmcf_approx_match_workspace_bytes", nb, nn_, mm)
    _lib.call("dmcf_approx_match", _ptr(a), _ptr(b), nb, nn_, mm, _counts_ptr(c1), _counts_ptr(c2), _ptr(match), _ptr(ws), nbytes,
              _stream())
    return match if batched else match[0]


def match_cost_backward(xyz1, xyz2, match, grad_cost, need1=True, need2=True):
    """dmcf_match_cost_backward: (grad_xyz1 [b, n, 3], grad_xyz2 [b, m, 3]) of ``match_cost`` for [b, n, 3] / [b, m, 3] sets, a
    dense match [b, m, n] and grad_cost [b] (None where not wanted)."""
    xyz1, xyz2 = _sets3(xyz1, xyz2)
    nb, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    dev = xyz1.device
    match = _dev_exact(match, "match", torch.float32, (nb, m, n), dev)
    gc = _dev_exact(grad_cost, "grad_cost", torch.float32, (nb,), dev)
    gx1 = torch.empty((nb, n, 3), dtype=torch.float32, device=dev) if need1 else None
    gx2 = torch.empty((nb, m, 3), dtype=torch.float32, device=dev) if need2 else None
    if nb > 0 and (need1 or need2):
        ws, nbytes = _workspace(dev, "dmcf_match_cost_backward_workspace_bytes", nb, n, m)
        _lib.call("dmcf_match_cost_backward", _ptr(xyz1), _ptr(xyz2), nb, n, m, _ptr(match), _ptr(gc), _ptr(gx1), _ptr(gx2),
                  _ptr(ws), nbytes, _stream())
    return gx1, gx2


class MatchCostFunction(torch.autograd.Function):
    """Autograd node of ``match_cost`` (MatchCostGrad, tf_approxmatch.cu:346-430): gradients for both point sets; the match
    gets none (approx_match has no gradient)."""

    @staticmethod
    def forward(ctx, a, b, mt):
        ctx.save_for_backward(a, b, mt)
        return _match_cost_impl(a, b, mt)

    @staticmethod
    def backward(ctx, grad_cost):
        a, b, mt = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need1 or need2):
            return None, None, None
        gx1, gx2 = match_cost_backward(a, b, mt, grad_cost, need1, need2)
        return gx1, gx2, None


def match_cost(xyz1, xyz2, match):
    """Mirror of ``utils/tools/tf_approxmatch.py: match_cost(xyz1, xyz2, match)`` -> cost [b] =
    sum_{l,k} match[l, k] |xyz2[l] - xyz1[k]| (dmcf_match_cost).  Differentiable in xyz1 and xyz2 (dmcf_match_cost_backward);
    the match is a constant."""
    a, b, batched = _pair_batch(xyz1, xyz2)
    nb, n, m = a.shape[0], a.shape[1], b.shape[1]
    mt = _dev_f32(match, "match").detach()
    if not batched:
        mt = mt.unsqueeze(0)
    if tuple(mt.shape) != (nb, m, n):
        raise ValueError(f"match must have shape {(nb, m, n) if batched else (m, n)}, got {tuple(match.shape)}")
    cost = MatchCostFunction.apply(a, b, mt) if _wants_grad(a, b) else _match_cost_impl(a, b, mt)
    return cost if batched else cost[0]


def _match_cost_impl(a, b, mt):
    nb, n, m = a.shape[0], a.shape[1], b.shape[1]
    cost = torch.empty(nb, dtype=torch.float32, device=a.device)
    ws, nbytes = _workspace(a.device, "dmcf_match_cost_workspace_bytes", nb, n, m)
    _lib.call("dmcf_match_cost", _ptr(a), _ptr(b), nb, n, m, _ptr(mt), _ptr(cost), _ptr(ws), nbytes, _stream())
    return cost


EMD_LEVELS = 10  # levels of the approximate match (dmcf_emd_with_levels records two ratios per point and level)


def _emd_impl(a, b, c1, c2, levels=None):
    nb, nn_, mm = a.shape[0], a.shape[1], b.shape[1]
    cost = torch.empty(nb, dtype=torch.float32, device=a.device)
    ws, nbytes = _workspace(a.device, "dmcf_emd_workspace_bytes", nb, nn_, mm)
    if levels is None:
        _lib.call("dmcf_emd", _ptr(a), _ptr(b), nb, nn_, mm, _counts_ptr(c1), _counts_ptr(c2), _ptr(cost), _ptr(ws), nbytes,
                  _stream())
    else:
        _lib.call("dmcf_emd_with_levels", _ptr(a), _ptr(b), nb, nn_, mm, _counts_ptr(c1), _counts_ptr(c2), _ptr(cost), _ptr(levels),
                  _ptr(ws), nbytes, _stream())
    return cost


def emd_with_levels(xyz1, xyz2, n=None, m=None):
    """dmcf_emd_with_levels on float32 GPU sets of shape exactly [b, n, 3] / [b, m, 3] -> (cost [b], levels [b, 10, n + m]): the
    cost of :func:`emd` (same bits) and, per level, ratioL after pass A ([:n]) and ratioR after pass B ([n:]), the state
    :func:`emd_backward` needs."""
    xyz1, xyz2 = _sets3(xyz1, xyz2)
    nb, nn_, mm = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    c1, c2 = _host_counts(n, nb, nn_, "n"), _host_counts(m, nb, mm, "m")
    levels = torch.empty((nb, EMD_LEVELS, nn_ + mm), dtype=torch.float32, device=xyz1.device)
    return _emd_impl(xyz1, xyz2, c1, c2, levels), levels


def emd_backward(xyz1, xyz2, levels, grad_cost, n=None, m=None, need1=True, need2=True):
    """dmcf_emd_backward: (grad_xyz1 [b, n, 3], grad_xyz2 [b, m, 3]) of :func:`emd` with the match held constant, from the
    ``levels`` of :func:`emd_with_levels` (same [b, n, 3] / [b, m, 3] sets and counts) and grad_cost [b], without forming the
    match; rows past a count are 0."""
    xyz1, xyz2 = _sets3(xyz1, xyz2)
    nb, nn_, mm = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    c1, c2 = _host_counts(n, nb, nn_, "n"), _host_counts(m, nb, mm, "m")
    dev = xyz1.device
    levels = _dev_exact(levels, "levels", torch.float32, (nb, EMD_LEVELS, nn_ + mm), dev)
    gc = _dev_exact(grad_cost, "grad_cost", torch.float32, (nb,), dev)
    gx1 = torch.empty((nb, nn_, 3), dtype=torch.float32, device=dev) if need1 else None
    gx2 = torch.empty((nb, mm, 3), dtype=torch.float32, device=dev) if need2 else None
    if nb > 0 and (need1 or need2):
        ws, nbytes = _workspace(dev, "dmcf_emd_backward_workspace_bytes", nb, nn_, mm)
        _lib.call("dmcf_emd_backward", _ptr(xyz1), _ptr(xyz2), nb, nn_, mm, _counts_ptr(c1), _counts_ptr(c2), _ptr(levels),
                  _ptr(gc), _ptr(gx1), _ptr(gx2), _ptr(ws), nbytes, _stream())
    return gx1, gx2


class EmdFunction(torch.autograd.Function):
    """Autograd node of :func:`emd`: the forward records the ratios of every level (dmcf_emd_with_levels, same cost bits as
    dmcf_emd), the backward is dmcf_emd_backward (match-free)."""

    @staticmethod
    def forward(ctx, a, b, c1, c2):
        levels = torch.empty((a.shape[0], EMD_LEVELS, a.shape[1] + b.shape[1]), dtype=torch.float32, device=a.device)
        cost = _emd_impl(a, b, c1, c2, levels)
        ctx.save_for_backward(a, b, levels)
        ctx.counts = (c1, c2)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        a, b, levels = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need1 or need2):
            return None, None, None, None
        c1, c2 = ctx.counts
        gx1, gx2 = emd_backward(a, b, levels, grad_cost, c1, c2, need1, need2)
        return gx1, gx2, None, None


def emd_row_splits(shape1, shape2, row_splits1, row_splits2, wants_grad=False, record=False):
    """The host-side checks of emd with row splits on the shapes of the two point sets, all of them before a device is
    touched, in the order of the other batched ops: both or neither and no gradient (NotImplementedError), then [n_total, 2|3]
    sets, well-formed splits and equal batch sizes (ValueError).  Unlike nn_distance, an item with an empty set is legal.
    ``record=True``: the caller records, so a wanted gradient is no refusal; everything else stays.
    -> (host splits 1, host splits 2)."""
    if row_splits1 is None or row_splits2 is None:
        raise NotImplementedError("batched emd needs both row_splits1 and row_splits2")
    if wants_grad and not record:
        raise NotImplementedError("batched emd has no backward unless it records (emd_ragged_recording): call it under no_grad, "
                                  "or per item without row splits")
    for shape, name in ((shape1, "xyz1"), (shape2, "xyz2")):
        if len(shape) != 2 or shape[-1] not in (2, 3):
            raise ValueError(f"{name} must have shape [n_total, 3] or [n_total, 2] with row splits, got {tuple(shape)}")
    s1 = _host_row_splits(row_splits1, "row_splits1")[0]
    s2 = _host_row_splits(row_splits2, "row_splits2")[0]
    _check_row_splits(s1, shape1[0], "row_splits1")
    _check_row_splits(s2, shape2[0], "row_splits2")
    if len(s1) != len(s2):
        raise ValueError(f"row_splits1 and row_splits2 must have equal lengths (batch + 1), got {len(s1)} and {len(s2)}")
    return s1, s2


def _emd_ragged_operands(xyz1, xyz2, row_splits1, row_splits2, record):
    """The checks of :func:`emd_ragged` in their order -> (a [1, n_total, 3], b [1, m_total, 3], host splits 1, host splits 2,
    whether a gradient is wanted)."""
    for t, name in ((xyz1, "xyz1"), (xyz2, "xyz2")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
    wants_grad = _wants_grad(xyz1, xyz2)
    s1, s2 = emd_row_splits(xyz1.shape, xyz2.shape, row_splits1, row_splits2, wants_grad, record=record)
    a, _ = _point_batch(xyz1, "xyz1")
    b, _ = _point_batch(xyz2, "xyz2")
    if a.device != b.device:
        raise ValueError("xyz1 and xyz2 must be on the same device")
    return a, b, s1, s2, wants_grad


def _host_i64(s):
    return (ctypes.c_int64 * len(s))(*s)


def _emd_ragged_impl(a, b, s1, s2, levels=None):
    batch = len(s1) - 1
    n, m, dev = a.shape[1], b.shape[1], a.device
    if n == 0 and m == 0:  # (every item empty: the library enqueues nothing and leaves cost alone)
        return torch.zeros(batch, dtype=torch.float32, device=dev)
    cost = torch.empty(batch, dtype=torch.float32, device=dev)
    h1, h2 = _host_i64(s1), _host_i64(s2)
    ws, nbytes = _workspace(dev, "dmcf_emd_ragged_workspace_bytes", n, h1, m, h2, batch)
    if levels is None:
        _lib.call("dmcf_emd_ragged", _ptr(a), n, h1, _ptr(b), m, h2, batch, _ptr(cost), _ptr(ws), nbytes, _stream())
    else:
        _lib.call("dmcf_emd_ragged_with_levels", _ptr(a), n, h1, _ptr(b), m, h2, batch, _ptr(cost), _ptr(levels), _ptr(ws), nbytes,
                  _stream())
    return cost


def emd_ragged(xyz1, xyz2, row_splits1, row_splits2):
    """emd over a RAGGED batch in one call (dmcf_emd_ragged: 62 launches whatever the batch): xyz1 [n_total, 3|2] and xyz2
    [m_total, 3|2] float32 GPU tensors, item b being xyz1[rs1[b]:rs1[b + 1]] against xyz2[rs2[b]:rs2[b + 1]]; the splits a
    sequence, a CPU or device int64 tensor or a :class:`RowSplits`.  -> cost [batch], every entry with the bits of
    ``emd(xyz1_b[None], xyz2_b[None])[0]``; an item with an empty set costs 0.  No gradient: inputs that require grad raise
    NotImplementedError; :func:`emd_ragged_recording` is the differentiable form."""
    a, b, s1, s2, _ = _emd_ragged_operands(xyz1, xyz2, row_splits1, row_splits2, False)
    return _emd_ragged_impl(a, b, s1, s2)


def _ragged_sets(xyz1, xyz2, row_splits1, row_splits2):
    """The operands of the ragged EMD's recording forward and backward: float32 GPU sets of shape exactly [n_total, 3] /
    [m_total, 3] on one device and well-formed host splits of equal lengths -> (a, b, s1, s2), the sets contiguous."""
    for t, name in ((xyz1, "xyz1"), (xyz2, "xyz2")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if t.dim() != 2 or t.shape[-1] != 3:
            raise ValueError(f"{name} must have shape [n_total, 3] here, got {tuple(t.shape)}")
    s1, s2 = emd_row_splits(xyz1.shape, xyz2.shape, row_splits1, row_splits2, record=True)
    a, _ = _point_batch(xyz1, "xyz1")
    b, _ = _point_batch(xyz2, "xyz2")
    if a.device != b.device:
        raise ValueError(f"xyz1 is on {a.device}, xyz2 on {b.device}")
    return a[0], b[0], s1, s2


def emd_ragged_with_levels(xyz1, xyz2, row_splits1, row_splits2):
    """dmcf_emd_ragged_with_levels on float32 GPU sets of shape exactly [n_total, 3] / [m_total, 3] -> (cost [batch], levels
    [10, n_total + m_total]): the cost of :func:`emd_ragged` (same bits) and, per level, ratioL of every row of xyz1 after
    finish step A ([:n_total]) and ratioR of every row of xyz2 after finish step B ([n_total:]), the state
    :func:`emd_ragged_backward` needs; zeros in the rows of an item with an empty set."""
    a, b, s1, s2 = _ragged_sets(xyz1, xyz2, row_splits1, row_splits2)
    return _emd_ragged_recorded(a.unsqueeze(0), b.unsqueeze(0), s1, s2)


def _emd_ragged_recorded(a, b, s1, s2):
    n, m = a.shape[1], b.shape[1]
    if n == 0 and m == 0:  # (nothing is written then: the zeros are ours)
        return _emd_ragged_impl(a, b, s1, s2), torch.zeros((EMD_LEVELS, 0), dtype=torch.float32, device=a.device)
    levels = torch.empty((EMD_LEVELS, n + m), dtype=torch.float32, device=a.device)
    return _emd_ragged_impl(a, b, s1, s2, levels), levels


def emd_ragged_backward(xyz1, xyz2, row_splits1, row_splits2, levels, grad_cost, need1=True, need2=True):
    """dmcf_emd_ragged_backward: (grad_xyz1 [n_total, 3], grad_xyz2 [m_total, 3]) of :func:`emd_ragged` with the match held
    constant, from the ``levels`` of :func:`emd_ragged_with_levels` (same sets and splits) and grad_cost [batch]; None where not
    wanted.  One table copy and at most 4 launches whatever the batch; item b's rows have the bits of :func:`emd_backward` on
    item b alone, the rows of an item whose other set is empty are zero."""
    a, b, s1, s2 = _ragged_sets(xyz1, xyz2, row_splits1, row_splits2)
    batch, n, m, dev = len(s1) - 1, a.shape[0], b.shape[0], a.device
    levels = _dev_exact(levels, "levels", torch.float32, (EMD_LEVELS, n + m), dev)
    gc = _dev_exact(grad_cost, "grad_cost", torch.float32, (batch,), dev)
    gx1 = torch.empty((n, 3), dtype=torch.float32, device=dev) if need1 else None
    gx2 = torch.empty((m, 3), dtype=torch.float32, device=dev) if need2 else None
    if (need1 or need2) and n + m > 0:
        h1, h2 = _host_i64(s1), _host_i64(s2)
        ws, nbytes = _workspace(dev, "dmcf_emd_ragged_backward_workspace_bytes", n, h1, m, h2, batch)
        _lib.call("dmcf_emd_ragged_backward", _ptr(a), n, h1, _ptr(b), m, h2, batch, _ptr(levels), _ptr(gc), _ptr(gx1), _ptr(gx2),
                  _ptr(ws), nbytes, _stream())
    return gx1, gx2


class EmdRaggedFunction(torch.autograd.Function):
    """Autograd node of :func:`emd_ragged_recording`: the forward records the ratios of every level
    (dmcf_emd_ragged_with_levels, same cost bits as dmcf_emd_ragged), the backward is dmcf_emd_ragged_backward (match-free)."""

    @staticmethod
    def forward(ctx, a, b, s1, s2):
        cost, levels = _emd_ragged_recorded(a, b, s1, s2)
        ctx.save_for_backward(a, b, levels)
        ctx.splits = (s1, s2)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        a, b, levels = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need1 or need2):
            return None, None, None, None
        s1, s2 = ctx.splits
        gx1, gx2 = emd_ragged_backward(a[0], b[0], s1, s2, levels, grad_cost.contiguous(), need1, need2)
        return (None if gx1 is None else gx1.unsqueeze(0)), (None if gx2 is None else gx2.unsqueeze(0)), None, None


def emd_ragged_recording(xyz1, xyz2, row_splits1, row_splits2):
    """:func:`emd_ragged`, differentiable in both point sets with the match held constant.  When grad mode is on and an input
    requires grad, the forward records (dmcf_emd_ragged_with_levels, 40 bytes per point more, same cost bits) and cost carries a
    grad_fn whose backward is one dmcf_emd_ragged_backward call; item b's gradient rows have the bits of
    ``emd(xyz1_b[None], xyz2_b[None])`` differentiated on the item alone.  When nothing wants a gradient it is
    :func:`emd_ragged`: the plain entry point runs.  All other checks are :func:`emd_ragged`'s, in their order."""
    a, b, s1, s2, wants_grad = _emd_ragged_operands(xyz1, xyz2, row_splits1, row_splits2, True)
    return EmdRaggedFunction.apply(a, b, s1, s2) if wants_grad else _emd_ragged_impl(a, b, s1, s2)


def emd(xyz1, xyz2, n=None, m=None, row_splits1=None, row_splits2=None):
    """``match_cost(xyz1, xyz2, approx_match(xyz1, xyz2, n, m))`` without forming the match (dmcf_emd): cost [b] in O(n + m)
    memory.  Same arguments as :func:`approx_match`.  Differentiable in xyz1 and xyz2 with the match held constant
    (dmcf_emd_backward); only then, when grad mode is on and an input requires grad, does the forward record the ratios of
    every level (dmcf_emd_with_levels, 40 (n + m) bytes per item more, same cost bits).

    ``row_splits1`` / ``row_splits2`` (both or neither, and then no ``n`` / ``m``): a RAGGED batch in one call
    (:func:`emd_ragged`), xyz1 [n_total, 3] and xyz2 [m_total, 3]; cost [batch] equals the call on every item alone bit for
    bit.  No gradient here: inputs that require grad raise NotImplementedError; :func:`emd_ragged_recording` is the
    differentiable form."""
    if row_splits1 is not None or row_splits2 is not None:
        if row_splits1 is not None and row_splits2 is not None and (n is not None or m is not None):
            raise ValueError("emd takes row splits or the point counts n / m of a padded batch, not both")
        return emd_ragged(xyz1, xyz2, row_splits1, row_splits2)  # (one split alone: its NotImplementedError)
    a, b, batched = _pair_batch(xyz1, xyz2)
    nb, nn_, mm = a.shape[0], a.shape[1], b.shape[1]
    c1, c2 = _host_counts(n, nb, nn_, "n"), _host_counts(m, nb, mm, "m")
    cost = EmdFunction.apply(a, b, c1, c2) if _wants_grad(a, b) else _emd_impl(a, b, c1, c2)
    return cost if batched else cost[0]


HIST_TILE_ROWS = 1024  # DMCF_HIST_TILE_ROWS: rows of each set per workgroup of dmcf_hist_pair_ragged's digit and count launches


def percentile_plan(count, q):
    """Where ``np.percentile(both, q, axis=0)`` looks in the sorted ``both`` of 2 ``count`` float32 values -> ``(k, k_next,
    gamma)``: the result is numpy's ``_lerp(sorted[k], sorted[k_next], gamma)`` in float32.  The plan depends on the count
    alone, which is why it is host arithmetic (it travels to dmcf_hist_pair_ragged in its table).

    numpy's arithmetic for float32 data (lib/_function_base_impl.py of numpy 2.x), restated: ``quant = np.true_divide(q,
    np.float32(100))``; the virtual index of the default method "linear" is ``(n - 1) * quant`` in float32 (numpy prefers
    this form to ``n * quant + (alpha + quant * (1 - alpha - beta)) - 1`` with alpha = beta = 1, the form of numpy 1.22 -
    1.26, which rounds differently); ``k = floor(virtual)``, ``k_next = k + 1``, both ``n - 1`` when ``virtual >= n - 1`` and
    both 0 when ``virtual < 0``; ``gamma = virtual - k`` as float32 (exact).  tests/test_hist_pair_abi.py holds this to the
    installed numpy bit for bit."""
    n = 2 * int(count)
    if n < 2:
        raise ValueError(f"percentile_plan needs count >= 1, got {count}")
    quant = np.true_divide(q, np.float32(100))
    virtual = np.float32(n - 1) * np.float32(quant)
    k = int(np.floor(virtual))
    k_next, gamma = k + 1, np.float32(virtual - np.floor(virtual))
    if virtual >= n - 1:
        k, k_next, gamma = n - 1, n - 1, np.float32(0)  # (equal neighbours: the weight does not matter)
    if virtual < 0:
        k, k_next, gamma = 0, 0, np.float32(0)
    return k, k_next, gamma


def hist_pair_ragged(x, y, row_splits=None, bin_size=25):
    """The percentiles and the two histograms of ``evaluation_helper.compare_dist(x, y, bin_size)`` for a RAGGED batch in one
    call (dmcf_hist_pair_ragged: 9 launches, one memset and one table copy whatever the batch; no host read in between).

    ``x``, ``y``: float32 device tensors [n_total, 3] sharing ``row_splits`` (the forms of :func:`nn_distance_ragged`; None:
    one item).  -> ``(percentiles, counts, offsets)``: percentiles [batch, 2, 3] float32 holds np.percentile(both, 5 | 95,
    axis=0) of every item's ``both = concatenate((x_b, y_b))``; counts is one int32 device tensor, item b's block being
    ``counts[offsets[b]:offsets[b + 1]]`` -- first the (per_b + 1)^3 bin counts of x_b in np.ravel_multi_index order, then
    those of y_b -- with ``per_b = int((cnt_b // bin_size) ** (1 / 3))``; offsets is a host list [batch + 1].  Everything is
    selected and summed in integers: the values are the host function's, bit for bit, and two calls give equal bits.

    Inputs must be finite: NaN is not checked for and is out of scope (the host function returns NaN percentiles for it).
    ValueError: x or y not a float32 [n, 3] device tensor, different shapes, malformed splits, an item without rows."""
    for t, name in ((x, "x"), (y, "y")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_cuda:
            what = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be a float32 device tensor of shape [n, 3], got {what}")
    if x.shape != y.shape:
        raise ValueError(f"x and y must have equal shapes, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.device != y.device:
        raise ValueError("x and y must be on the same device")
    if bin_size < 1:
        raise ValueError(f"bin_size must be positive, got {bin_size}")
    n = int(x.shape[0])
    rs = (0, n) if row_splits is None else _host_row_splits(row_splits, "row_splits")[0]
    _check_row_splits(rs, n, "row_splits")
    batch = len(rs) - 1
    plan = (_lib.HistPlan * batch)()
    offsets = [0]
    for b in range(batch):
        cnt = rs[b + 1] - rs[b]
        if cnt < 1:
            raise ValueError(f"hist_pair_ragged needs non-empty items: item {b} has no rows")
        per = int((cnt // bin_size) ** (1 / 3))  # compare_dist's bin_cnt_per_dim; the clip's upper end adds one bin per axis
        k5, k5n, g5 = percentile_plan(cnt, 5)
        k95, k95n, g95 = percentile_plan(cnt, 95)
        plan[b].per = per
        plan[b].rank[:] = [k5, k5n, k95, k95n]
        plan[b].gamma[:] = [g5, g95]
        offsets.append(offsets[-1] + 2 * (per + 1) ** 3)
    x, y = x.contiguous(), y.contiguous()
    dev = x.device
    bins_total = offsets[-1] // 2
    percentiles = torch.empty((batch, 2, 3), dtype=torch.float32, device=dev)
    counts = torch.empty(offsets[-1], dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(dev, "dmcf_hist_pair_ragged_workspace_bytes", n, batch, bins_total)
    h = (ctypes.c_int64 * (batch + 1))(*rs)
    _lib.call("dmcf_hist_pair_ragged", _ptr(x), _ptr(y), n, h, batch, plan, bins_total, _ptr(percentiles), _ptr(counts), _ptr(ws),
              nbytes, _stream())
    return percentiles, counts, offsets


def _adam_args(params, grads, ms, vs, lr, beta_1, beta_2, epsilon, beta_1_power, beta_2_power, clip_norm):
    """-> (dmcf_adam_args, host table, [params, grads, ms, vs]) for :func:`adam_step` (device_tensors not yet set)."""
    if not (len(params) == len(grads) == len(ms) == len(vs)):
        raise ValueError("params, grads, m and v must have one entry each per tensor")
    recs = (_lib.AdamTensor * max(len(params), 1))()
    for i, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
        for t, name in ((p, "param"), (g, "grad"), (m, "m"), (v, "v")):
            _dev_f32(t, name)
            if not t.is_contiguous():
                raise ValueError(f"{name} of tensor {i} must be contiguous")
            if t.numel() != p.numel():
                raise ValueError(f"tensor {i}: param, grad, m and v must have the same number of elements")
        recs[i].param, recs[i].grad, recs[i].m, recs[i].v = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        recs[i].n = p.numel()
    a = _lib.AdamArgs()
    a.struct_size = ctypes.sizeof(_lib.AdamArgs)
    a.n_tensors = len(params)
    a.tensors = ctypes.cast(recs, ctypes.c_void_p).value
    a.lr, a.beta_1, a.beta_2, a.epsilon = float(lr), float(beta_1), float(beta_2), float(epsilon)
    a.beta_1_power, a.beta_2_power = float(beta_1_power), float(beta_2_power)
    a.clip_norm = float(clip_norm) if clip_norm is not None else -1.0
    return a, recs


def adam_step_kernel_names(params, grads, ms, vs, clip_norm=None):
    """';'-separated names of the kernels dmcf_adam_step launches for these tensors (rocprofv3's kernel names)."""
    a, recs = _adam_args(params, grads, ms, vs, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, clip_norm)
    a.device_tensors = 1 if len(params) else None  # (validated for presence only: nothing is read)
    return _kernel_name("dmcf_adam_step_kernel_names", ctypes.byref(a), size=64).decode()


def adam_step(params, grads, ms, vs, lr, beta_1, beta_2, epsilon, beta_1_power, beta_2_power, clip_norm=None):
    """dmcf_adam_step: one Adam update of every (param, grad, m, v) in place, in the order of operations of TensorFlow's
    ApplyAdam (``alpha = lr sqrt(1 - beta_2_power) / (1 - beta_1_power)``, ``param -= alpha m / (epsilon + sqrt(v))``), each
    gradient clipped per tensor to ``clip_norm`` first when that is > 0 (tf.clip_by_norm).  Lists of contiguous float32 device
    tensors; the scalars are Keras' coefficients for the iteration (utils/tools/losses.KerasAdam computes them).  One launch
    (two with clipping); the descriptor table goes to the device in one copy."""
    a, recs = _adam_args(params, grads, ms, vs, lr, beta_1, beta_2, epsilon, beta_1_power, beta_2_power, clip_norm)
    if not params:
        return
    dev = params[0].device
    raw = torch.frombuffer(bytearray(ctypes.string_at(recs, ctypes.sizeof(_lib.AdamTensor) * len(params))), dtype=torch.uint8)
    table = raw.to(dev, non_blocking=False)
    a.device_tensors = table.data_ptr()
    ws, nbytes = _workspace(dev, "dmcf_adam_step_workspace_bytes", ctypes.byref(a), least=8)
    t0 = timer.begin() if timer is not None else None
    _lib.call("dmcf_adam_step", ctypes.byref(a), _ptr(ws), nbytes, _stream())
    if timer is not None:
        timer.end("adam_step", dict(tensors=len(params), kernel=adam_step_kernel_names(params, grads, ms, vs, clip_norm)), t0)
    # (the table and the workspace are freed into torch's caching allocator, which keeps them from reuse until the stream has
    # passed this point)
    del table, ws


def raster_discs(xy, radius, color_argb, width, height, out=None):
    """Draw filled, anti-aliased discs of one colour (dmcf_raster_count / dmcf_raster_discs; the pixel model is in
    include/dmcf_hip.h) into ``out``, float32 RGB ``[F, H, W, 3]`` in [0, 1], composited in place; ``out=None``: a new white
    image.  ``xy``: float32 CUDA ``[F, N, 2]`` (frame f's points into frame f) or ``[N, 2]`` (the same points in every frame,
    binned once) in pixel coordinates; ``radius`` in pixels; ``color_argb`` 0xAARRGGBB.  Returns ``out``.  The two calls
    bracket one host read of the bin size."""
    L = _lib.lib()
    if not isinstance(xy, torch.Tensor):
        raise TypeError("xy must be a torch tensor")
    if xy.dim() not in (2, 3) or xy.shape[-1] != 2:
        raise ValueError(f"xy must have shape [F, N, 2] or [N, 2], got {tuple(xy.shape)}")
    width, height, color_argb = int(width), int(height), int(color_argb)
    if width <= 0 or height <= 0:
        raise ValueError(f"width and height must be positive, got {width} x {height}")
    if not 0 <= color_argb <= 0xFFFFFFFF:
        raise ValueError(f"color_argb must be a 32-bit ARGB value, got {color_argb:#x}")
    xy = _dev_f32(xy, "xy")
    if out is None:
        frames = xy.shape[0] if xy.dim() == 3 else 1
        out = torch.ones((frames, height, width, 3), dtype=torch.float32, device=xy.device)
    else:
        _dev_f32(out, "out")
        if out.device != xy.device:
            raise ValueError(f"out is on {out.device}, xy on {xy.device}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous (it is written in place)")
        if out.dim() != 4 or tuple(out.shape[1:]) != (height, width, 3):
            raise ValueError(f"out must have shape [F, {height}, {width}, 3], got {tuple(out.shape)}")
    frames = out.shape[0]
    if xy.dim() == 3 and xy.shape[0] != frames:
        raise ValueError(f"xy holds {xy.shape[0]} frames, out {frames}")
    n = xy.shape[-2]
    stride = n if xy.dim() == 3 else 0
    radius = float(radius)
    if n == 0 or frames == 0 or not (np.isfinite(radius) and radius > 0.0) or (color_argb >> 24) == 0:
        return out  # nothing is drawn (the library would not launch either)
    nbytes = int(L.dmcf_raster_workspace_bytes(n, frames, stride, width, height))
    if nbytes == 0:
        raise ValueError(f"dmcf_raster: unsupported size (n={n}, frames={frames}, {width} x {height})")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xy.device)
    total = torch.empty(1, dtype=torch.int64, device=xy.device)
    _lib.call("dmcf_raster_count", _ptr(xy), n, frames, stride, radius, width, height, _ptr(ws), nbytes, _ptr(total), _stream())
    cap = int(total.item())
    bins = torch.empty((max(cap, 1), 2), dtype=torch.float32, device=xy.device)
    _lib.call("dmcf_raster_discs", _ptr(xy), n, frames, stride, radius, color_argb, width, height, _ptr(out), _ptr(ws), nbytes,
              _ptr(bins), cap, _stream())
    return out


def rgba8(image):
    """float RGB ``[..., 3]`` in [0, 1] -> uint8 RGBA ``[..., 4]``: ``round(255 C)`` (half to even), clamped to [0, 255], alpha
    255."""
    q = torch.clamp(torch.round(image * 255.0), 0.0, 255.0).to(torch.uint8)
    return torch.cat([q, torch.full_like(q[..., :1], 255)], dim=-1)


Camera = collections.namedtuple("Camera", ["view", "focal", "cx", "cy", "near", "orthographic"])
Camera.__doc__ = """struct dmcf_camera (include/dmcf_hip.h): ``view`` 12 floats, the row-major 3 x 4 world -> camera matrix (the
camera looks along +z, x is right, y is down); ``focal`` pixels per world unit at z = 1 (per world unit when ``orthographic``);
``(cx, cy)`` the principal point; ``near`` >= 0.  :func:`look_at` builds one."""

SplatLayer = collections.namedtuple("SplatLayer", ["keys", "xyz", "radius", "color_argb", "farthest"], defaults=(False,))
SplatLayer.__doc__ = """One point group of :func:`splat_shade`: the ``keys`` :func:`splat_depth` left for ``xyz`` at ``radius``
(with the same ``farthest``), and the group's colour 0xAARRGGBB."""


def look_at(eye, target, up, width, height, fov_deg=35.0, ortho_height=None, near=1e-3):
    """A :class:`Camera` at ``eye`` looking at ``target`` with ``up`` pointing up in the image, for a ``width`` x ``height``
    image: the principal point is the image centre; ``focal = 0.5 height / tan(fov / 2)`` (``fov_deg`` the vertical field of
    view), or ``height / ortho_height`` for an orthographic camera showing ``ortho_height`` world units from top to bottom.
    The view matrix is formed in float64 and rounded to float32 once.  Degenerate input (``eye == target``, ``up`` parallel to
    the view direction, values that are not finite) is a ValueError."""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (eye, target, up))
    if eye.shape != (3,) or target.shape != (3,) or up.shape != (3,):
        raise ValueError("eye, target and up must have 3 components each")
    if not (np.isfinite(eye).all() and np.isfinite(target).all() and np.isfinite(up).all()):
        raise ValueError("eye, target and up must be finite")
    width, height, near = int(width), int(height), float(near)
    if width <= 0 or height <= 0:
        raise ValueError(f"width and height must be positive, got {width} x {height}")
    if not (np.isfinite(near) and near >= 0.0):
        raise ValueError(f"near must be finite and >= 0, got {near}")
    forward = target - eye
    dist = np.linalg.norm(forward)
    if not dist > 0.0:
        raise ValueError("eye and target coincide: there is no view direction")
    forward = forward / dist
    right = np.cross(forward, up)
    rn, un = np.linalg.norm(right), np.linalg.norm(up)
    if not (un > 0.0 and rn > 1e-12 * un):
        raise ValueError("up is zero or parallel to the view direction")
    right = right / rn
    down = np.cross(forward, right)  # x right, y down, z forward: a right-handed frame
    rows = np.stack([right, down, forward])
    view = np.concatenate([rows, -(rows @ eye)[:, None]], axis=1)
    if ortho_height is None:
        fov = float(fov_deg)
        if not 0.0 < fov < 180.0:
            raise ValueError(f"fov_deg must lie in (0, 180), got {fov_deg}")
        focal = 0.5 * height / np.tan(np.deg2rad(fov) / 2.0)
    else:
        if not (np.isfinite(ortho_height) and ortho_height > 0.0):
            raise ValueError(f"ortho_height must be positive, got {ortho_height}")
        focal = height / float(ortho_height)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    return Camera(tuple(f32(v) for v in view.reshape(-1)), f32(focal), f32(0.5 * width), f32(0.5 * height), f32(near),
                  ortho_height is not None)


def _camera_struct(camera):
    if not isinstance(camera, Camera):
        raise TypeError("camera must be an ops.Camera (see ops.look_at)")
    if len(camera.view) != 12:
        raise ValueError(f"camera.view must hold 12 values (3 x 4, row-major), got {len(camera.view)}")
    c = _lib.Camera()
    c.view = (ctypes.c_float * 12)(*[float(v) for v in camera.view])
    c.focal, c.cx, c.cy, c.near = float(camera.focal), float(camera.cx), float(camera.cy), float(camera.near)
    c.orthographic = 1 if camera.orthographic else 0
    vals = list(c.view) + [c.focal, c.cx, c.cy, c.near]
    if not (np.isfinite(vals).all() and c.focal > 0.0 and c.near >= 0.0):
        raise ValueError("camera: every value must be finite, focal > 0 and near >= 0")
    return c


def _splat_sizes(width, height, min_px):
    width, height, min_px = int(width), int(height), float(min_px)
    if width <= 0 or height <= 0 or width > 32768 or height > 32768:
        raise ValueError(f"width and height must lie in [1, 32768], got {width} x {height}")
    if not (np.isfinite(min_px) and min_px >= 0.0):
        raise ValueError(f"min_px must be finite and >= 0, got {min_px}")
    return width, height, min_px


def _splat_points(xyz, name):
    if not isinstance(xyz, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if xyz.dim() not in (2, 3) or xyz.shape[-1] != 3:
        raise ValueError(f"{name} must have shape [F, N, 3] or [N, 3], got {tuple(xyz.shape)}")
    return _dev_f32(xyz, name)


def _splat_keys(keys, name, device, shape):
    if not isinstance(keys, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if keys.dtype != torch.int64:
        raise TypeError(f"{name} must be int64 (the uint64 keys' bits), got {keys.dtype}")
    if not keys.is_cuda:
        raise _lib.DmcfError(f"{name} is on {keys.device}: the splat runs on the GPU only (no CPU fallback)")
    if keys.device != device:
        raise ValueError(f"{name} is on {keys.device}, the points on {device}")
    if not keys.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if keys.dim() != 3 or (shape is not None and tuple(keys.shape[1:]) != shape):
        want = f"[F, {shape[0]}, {shape[1]}]" if shape is not None else "[F, H, W]"
        raise ValueError(f"{name} must have shape {want}, got {tuple(keys.shape)}")
    return keys


def splat_depth(xyz, radius, camera, width, height, farthest=False, min_px=0.75, out=None):
    """The depth pass of the sphere splat (dmcf_splat_depth; pixel model in include/dmcf_hip.h): per pixel the key
    ``(bits(z) << 32) | index`` of the nearest sphere of ``xyz`` -- of the farthest one, with the depth word complemented, when
    ``farthest`` -- minimised into ``out``.  ``xyz``: float32 CUDA ``[F, N, 3]`` (frame f's points into frame f) or ``[N, 3]``
    (the same points into every frame); ``radius`` in world units; ``min_px`` the smallest radius in pixels a sphere is drawn
    with.  ``out``: int64 ``[F, H, W]`` holding the uint64 keys' bits, -1 = empty; it fixes the frame count, is NOT cleared (so
    several groups can share it), and is created filled with -1 when None.  Returns ``out``.  One launch, no host read."""
    width, height, min_px = _splat_sizes(width, height, min_px)
    cam = _camera_struct(camera)
    xyz = _splat_points(xyz, "xyz")
    if out is None:
        frames = xyz.shape[0] if xyz.dim() == 3 else 1
        out = torch.full((frames, height, width), -1, dtype=torch.int64, device=xyz.device)
    else:
        _splat_keys(out, "out", xyz.device, (height, width))
    frames = out.shape[0]
    if xyz.dim() == 3 and xyz.shape[0] != frames:
        raise ValueError(f"xyz holds {xyz.shape[0]} frames, out {frames}")
    if frames > 65535:
        raise ValueError(f"at most 65535 frames per call, got {frames}")
    n = xyz.shape[-2]
    stride = n if xyz.dim() == 3 else 0
    radius = float(radius)
    if n == 0 or frames == 0 or not (np.isfinite(radius) and radius > 0.0):
        return out  # nothing is splatted (the library would not launch either)
    _lib.call("dmcf_splat_depth", _ptr(xyz), n, frames, stride, radius, min_px, ctypes.byref(cam), width, height,
              _lib.SPLAT_FARTHEST if farthest else 0, _ptr(out), _stream())
    return out


def splat_shade(layers, camera, width, height, out=None, ambient=0.3, min_px=0.75, return_depth=False):
    """The shade pass of the sphere splat (dmcf_splat_shade): per pixel the layer with the smallest depth wins (ties: the
    earlier layer), and its sphere is shaded ``ambient + (1 - ambient) nz`` and composited with the layer colour's alpha into
    ``out``, float32 RGB ``[F, H, W, 3]`` in [0, 1], in place; ``out=None``: a new white image.  ``layers``: up to 4
    :class:`SplatLayer`, each with the ``xyz``, ``radius`` and ``farthest`` its ``keys`` were made with; ``camera`` and
    ``min_px`` as in those calls.  Pixels without a sample keep what ``out`` holds.  Returns ``out``, or ``(out, depth)`` with
    ``depth`` float32 ``[F, H, W]`` (+inf where there is no sample) when ``return_depth``.  One launch.  ``ops.rgba8`` turns
    the result into 8-bit RGBA."""
    layers = list(layers)
    if len(layers) > _lib.SPLAT_MAX_LAYERS:
        raise ValueError(f"at most {_lib.SPLAT_MAX_LAYERS} layers per call, got {len(layers)}")
    if not layers and out is None:
        raise ValueError("splat_shade needs a layer or an image to tell the device and the frame count")
    width, height, min_px = _splat_sizes(width, height, min_px)
    ambient = float(ambient)
    if not 0.0 <= ambient <= 1.0:
        raise ValueError(f"ambient must lie in [0, 1], got {ambient}")
    cam = _camera_struct(camera)
    recs = (_lib.SplatLayer * max(len(layers), 1))()
    keep = []  # (tensors whose pointers sit in recs)
    device = out.device if isinstance(out, torch.Tensor) else None
    frames = None
    for j, layer in enumerate(layers):
        if not isinstance(layer, SplatLayer):
            raise TypeError(f"layers[{j}] must be an ops.SplatLayer")
        xyz = _splat_points(layer.xyz, f"layers[{j}].xyz")
        device = xyz.device if device is None else device
        keys = _splat_keys(layer.keys, f"layers[{j}].keys", device, (height, width))
        if xyz.device != device:
            raise ValueError(f"layers[{j}].xyz is on {xyz.device}, expected {device}")
        frames = keys.shape[0] if frames is None else frames
        if keys.shape[0] != frames or (xyz.dim() == 3 and xyz.shape[0] != frames):
            raise ValueError(f"layers[{j}]: {keys.shape[0]} frames of keys, {tuple(xyz.shape)} points, expected {frames} frames")
        color = int(layer.color_argb)
        if not 0 <= color <= 0xFFFFFFFF:
            raise ValueError(f"layers[{j}].color_argb must be a 32-bit ARGB value, got {color:#x}")
        r = recs[j]
        r.keys, r.xyz = keys.data_ptr(), xyz.data_ptr()
        r.n_points = xyz.shape[-2]
        r.frame_stride = r.n_points if xyz.dim() == 3 else 0
        r.radius, r.color_argb = float(layer.radius), color
        r.flags = _lib.SPLAT_FARTHEST if layer.farthest else 0
        keep.append((keys, xyz))
    if out is None:
        out = torch.ones((frames, height, width, 3), dtype=torch.float32, device=device)
    else:
        _dev_f32(out, "out")
        if out.device != device:
            raise ValueError(f"out is on {out.device}, the layers on {device}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous (it is written in place)")
        if out.dim() != 4 or tuple(out.shape[1:]) != (height, width, 3):
            raise ValueError(f"out must have shape [F, {height}, {width}, 3], got {tuple(out.shape)}")
        if frames is not None and out.shape[0] != frames:
            raise ValueError(f"out holds {out.shape[0]} frames, the layers {frames}")
    frames = out.shape[0]
    if frames > 65535:
        raise ValueError(f"at most 65535 frames per call, got {frames}")
    depth = torch.empty((frames, height, width), dtype=torch.float32, device=out.device) if return_depth else None
    if frames:
        _lib.call("dmcf_splat_shade", recs, len(layers), ctypes.byref(cam), min_px, ambient, width, height, frames, _ptr(out),
                  _ptr(depth), _stream())
    del keep
    return (out, depth) if return_depth else out


SPH1D_MAX_POINTS = 64  # dmcf_sph1d_rollout: one 64-lane wavefront per scene, lane = point
SPH1D_LAUNCH_ITERS = 100_000  # worst-case solver iterations (frames * max_iter) one launch may cover: about 1 s at 64 points


def sph1d_rollout(state, n_tot, frames, h, rest_dens, stiffness, visc, gravity, dt, eps=0.01, max_iter=10000, bcnt=2,
                  launch_iters=SPH1D_LAUNCH_ITERS):
    """``frames`` steps of the reference's 1-D SPH solver (SPH1D.step, datasets/column_gen.py:159-186) for a batch of
    independent scenes (dmcf_sph1d_rollout; formulas and precision in include/dmcf_hip.h).

    ``state``: float32 CUDA ``[S, P, 3]`` = (position, velocity, mass) per point as ``SPH1D.setup`` lays it out, the ``bcnt``
    boundary points first; scene ``s`` holds ``n_tot[s]`` points (``n_tot``: int32 CUDA ``[S]``, or a sequence of ints), the
    rest of its slot is padding.  ``P > 64`` raises NotImplementedError (a scene is one wavefront).  Returns
    ``(sequence [frames, S, P, 2], state_out [S, P, 3], iterations [frames, S] int32)``: (position, velocity) BEFORE each
    step, the state after the last one, and the pressure iterations every step took.

    The rollout is cut into launches of ``max(1, launch_iters // max_iter)`` frames, so that no launch covers more than
    ``launch_iters`` solver iterations in the worst case (one frame's ``max_iter`` cannot be cut further); the state is carried
    from launch to launch, and the result has the bits of a single launch."""
    state = _dev_f32(state, "state")
    if state.dim() != 3 or state.shape[2] != 3:
        raise ValueError(f"state must have shape [S, P, 3], got {tuple(state.shape)}")
    S, P = int(state.shape[0]), int(state.shape[1])
    if P > SPH1D_MAX_POINTS:
        raise NotImplementedError(f"sph1d_rollout: a scene of {P} points (boundary included) exceeds the limit of "
                                  f"{SPH1D_MAX_POINTS}: the solver runs one 64-lane wavefront per scene")
    frames, max_iter, bcnt = int(frames), int(max_iter), int(bcnt)
    if frames < 0 or max_iter < 1 or P < 1 or not 0 <= bcnt < P:
        raise ValueError(f"sph1d_rollout: frames={frames}, max_iter={max_iter}, bcnt={bcnt}, P={P}")
    if not isinstance(n_tot, torch.Tensor):
        n_tot = torch.as_tensor(np.asarray(n_tot, dtype=np.int32), device=state.device)
    if n_tot.dtype != torch.int32 or n_tot.device != state.device or tuple(n_tot.shape) != (S,):
        raise ValueError(f"n_tot must be int32 [{S}] on {state.device}, got {n_tot.dtype} {tuple(n_tot.shape)} on {n_tot.device}")
    n_tot = n_tot.contiguous()
    p = _lib.Sph1dParams()
    p.struct_size = ctypes.sizeof(p)
    p.bcnt, p.max_iter = bcnt, max_iter
    p.h, p.rest_dens, p.stiffness, p.visc = float(h), float(rest_dens), float(stiffness), float(visc)
    p.gravity, p.dt, p.eps = float(gravity), float(dt), float(eps)
    seq = torch.empty((frames, S, P, 2), dtype=torch.float32, device=state.device)
    iters = torch.empty((frames, S), dtype=torch.int32, device=state.device)
    out = state.clone()  # advanced in place, launch by launch
    if S == 0:
        return seq, out, iters
    per = max(1, int(launch_iters) // max_iter)
    for t0 in range(0, max(frames, 1), per):
        k = min(per, frames - t0)
        _lib.call("dmcf_sph1d_rollout", _ptr(out), _ptr(n_tot), S, P, ctypes.byref(p), k, _ptr(seq[t0:]) if k else None, _ptr(out),
                  _ptr(iters[t0:]) if k else None, _stream())
    return seq, out, iters
