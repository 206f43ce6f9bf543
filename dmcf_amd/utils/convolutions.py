"""ContinuousConv layer -- mirror of the reference's ``utils/convolutions.py:34-473`` on PyTorch-ROCm.

Same constructor keywords (convolutions.py:150-175), same ``call`` signature (:277-286), same side
attributes read by callers (``.nns``, ``._avg_neighbors``, ``._conv_values``, ``._conv_output``), same
weight names (``kernel``, ``bias``), so the model code and configs of the reference drop onto it.
What differs is underneath: the radius search, the window function, the CConv itself and the whole
ASCC body (mirror + two continuous_conv calls + batched matmul, :410-412,:433-458) are one HIP
search + one HIP kernel launch each (dmcf_amd/ops.py -> libdmcf_hip.so).

Weights are built with ``requires_grad=False``: inference records no autograd history.  After
``layer.requires_grad_(True)`` (or with input features that require grad) a call records it and takes
the neighbour-list form, whose backward is dmcf_cconv_backward (``ContinuousConv._forward_train``).  Extents of rank 1, one
per output point, record only in a layer built with ``record_per_point_extents=True`` (dmcf_cconv_backward_extents); any
other layer refuses them while recording, as before.

``SparseConv`` and ``SparseConvTranspose`` (the reference's :476-885) sit on a path of their own: a max-norm search
(``ops.FixedRadiusSearch(metric="Linf")``) and the voxel-convolution kernel (``ops.sparse_conv`` / ``ops.sparse_conv_transpose``).
"""
import math
import os
import threading

import numpy as np
import torch

from .. import ops
from .tools.losses import WindowFunction

__all__ = ["ContinuousConv", "SparseConv", "SparseConvTranspose", "neighbor_cache"]

# dmcf_cconv_scatter_forward (splat S) is taken for particles -> coarse-lattice layers with these output channel counts (8 is
# implemented and tested but measures slower than the gather kernels: tools/bench_scatter.py) ...
SCATTER_OUT_CHANNELS = (4,)
SCATTER_MIN_INPUTS = 4096           # ... for point sets big enough to fill the device (small scenes are paced by launches),
SCATTER_MAX_LATTICE_CELLS = 1 << 16  # and lattices whose cell coordinates stay exact in float32 arithmetic
SMALL_LIST_ENTRIES = 1 << 21  # padded lists up to this size stay padded whatever their fill (see _NeighborCache.search: 4 total + 2^22)


class _NeighborCache:
    """Per-step reuse of neighbour lists and grids.

    The reference runs its own FixedRadiusSearch inside every ContinuousConv.call
    (convolutions.py:354-358), 18/27/43 searches per step of which only 12/12/19 are distinct
    (SURVEY.md section 3.2).  Inside ``with neighbor_cache():`` a search is keyed by
    (points, queries, radius, ignore_query_point) -- tensors by storage identity -- and computed once;
    the cell-sorted grid of a point set is shared between searches with the same radius.
    Results are identical to searching again (same inputs, deterministic kernel)."""

    def __init__(self):
        self.depth = 0
        # longest-row estimates from the previous step, by WHAT the search is (radius, size class of both point sets, its
        # flags -- _hint_key): with them a step enqueues all its searches without a single host round trip (see search()).
        # (Keyed by the position in the step's sequence of searches through round 3: when a layer between two lattices fell
        # back to a neighbour list in the middle of a rollout, every later search took its neighbour's estimate -- a 35-entry
        # stride for a 286-entry list -- and the step was repeated.)
        self.hints = {}
        self.caps = {}  # (class, n-th search of that class in the step) -> entries of its padded buffers in the previous step
        self.totals = {}  # same keys -> pairs of that list in the previous step (padded rows or CSR: see search())
        self.last_overflow = []  # diagnostics: the lists that outgrew their estimates in the last step that had to be repeated
        # consumers per list: learnt in one step, used in the next to hand a list's buffers back to the allocator as soon
        # as its last consumer has enqueued its kernel (12 lists of 2.4 - 3.4 GB each at 1M particles; all of them alive
        # until the end of the step was 160 GB at 4M particles and sent the caching allocator into free / malloc cycles)
        self.expect = {}
        self.uses = {}
        self.slot_of = {}
        self.done = []
        self.use_hints = False
        self.nth = {}  # searches of each class so far in this step (the second half of a list's key in expect / uses / caps)
        self.pending = []
        self.reports = []  # (int64 device tensor, callback(list) -> outgrown?) read with the step's one synchronisation (report())
        self.lists = {}
        self.tables = {}
        self.plans = {}
        self.keepalive = []
        self.key = None
        self.states = {}  # key -> (hints, caps, expect) of the rollouts that are not the current one

    def select(self, key):
        """Swap in the estimates (hints / caps / expect) of ``key`` (outermost scope only)."""
        if key == self.key:
            return
        self.states[self.key] = (self.hints, self.caps, self.expect, self.totals)
        while len(self.states) > 16:  # a handful of (model, scene) rollouts at a time
            self.states.pop(next(iter(self.states)))
        self.hints, self.caps, self.expect, self.totals = self.states.pop(key, ({}, {}, {}, {}))
        self.key = key

    def __enter__(self):
        if self.depth == 0:
            self.nth = {}
            self.pending = []
            self.reports = []
        self.depth += 1
        return self

    def report(self, values, callback):
        """Device numbers somebody wants on the host when the step ends (int64 tensor; read in the step's single synchronisation,
        no round trip of their own): ``callback(list of ints)`` returns True if they show an estimated capacity outgrown -- the
        step is then repeated like one with an outgrown neighbour list.  Outside a step: read at once."""
        if self.depth == 0:
            return bool(callback(values.flatten().tolist()))
        self.reports.append((values.flatten().long(), callback))
        return False

    def __exit__(self, exc_type, exc, tb):
        self.depth -= 1
        if self.depth == 0:
            pending, self.pending = self.pending, []
            self._flush()
            for _, _, r in pending:  # layers keep their last list in .nns: do not let that pin the buffers into the next step
                r.release()
            if exc_type is None:
                self.expect = dict(self.uses)
            self._maxc = None
            self.uses = {}
            self.slot_of = {}
            from .. import lattice
            lattice.clear()
            self.lists.clear()
            self.tables.clear()
            self.plans.clear()
            self.keepalive.clear()
            reports, self.reports = self.reports, []
            outgrown = False
            if exc_type is None and reports:
                flat = torch.cat([v for v, _ in reports]).tolist()
                at = 0
                for v, cb in reports:
                    outgrown = bool(cb(flat[at: at + v.shape[0]])) or outgrown
                    at += v.shape[0]
            if exc_type is None and outgrown and not pending:
                raise ops.NeighborCapacityExceeded("an estimated capacity was outgrown; repeat the step")
            if exc_type is None and pending:
                # one synchronisation per step: validate the estimated capacities, refresh the estimates (the longest row and
                # the number of pairs of every list)
                # (the padded lists' numbers are gathered by four small launches for all of them, not three per list)
                pad = [k for k, (_, _, r) in enumerate(pending) if isinstance(r, ops.PaddedNeighborList)]
                oth = [k for k, (_, _, r) in enumerate(pending) if not isinstance(r, ops.PaddedNeighborList)]
                parts = []
                if pad:
                    parts.append(torch.cat([pending[k][2].max_count for k in pad]).long())
                    # (a list whose padded rows are small never takes the estimated-CSR form, so its pair count is not needed: no
                    # reduction launch for it -- ten per step of the 2-D models)
                    small = [pending[k][2].row_count.shape[0] * pending[k][2].stride <= SMALL_LIST_ENTRIES for k in pad]
                    zero = ops.const_tensor([0], torch.int64, pending[pad[0]][2].row_count.device)[0]
                    parts.append(torch.stack([zero if sm else pending[k][2].total_ref.long() for k, sm in zip(pad, small)]))
                for k in oth:
                    rs = pending[k][2].neighbors_row_splits
                    parts.append(torch.stack([torch.diff(rs).max() if rs.shape[0] > 1 else rs.new_zeros(()), rs[-1]]))
                flat = torch.cat(parts).tolist()
                vals = [None] * len(pending)
                for i, k in enumerate(pad):
                    vals[k] = (flat[i], None if small[i] else flat[len(pad) + i])
                for i, k in enumerate(oth):
                    vals[k] = (flat[2 * len(pad) + 2 * i], flat[2 * len(pad) + 2 * i + 1])
                fresh, tot = {}, {}
                over = []
                for (hkey, slot, r), (mx, total) in zip(pending, vals):
                    if isinstance(r, ops.PaddedNeighborList):
                        if r.overflowed(mx):
                            over.append((hkey, "row", r.stride, int(mx)))
                    elif r.overflowed(total):
                        over.append((hkey, "pairs", r.capacity, int(total)))
                    fresh[hkey] = max(fresh.get(hkey, 0), int(mx))  # (searches of one class share the longest of their rows)
                    if total is not None:
                        tot[slot] = int(total)
                # estimates come from the PREVIOUS step only: a class this step did not search is forgotten (its next search runs
                # the exact two passes once).  Keeping old entries let one search inherit another's: in the dam break the
                # lattices grow through the half-octave size classes, and at step 81 the s0 -> s2 list (2,300-entry rows)
                # arrived in the class the s2 -> s1 list (300) had left 30 steps earlier -- a repeated step.
                self.hints.clear()
                self.hints.update(fresh)
                self.totals.clear()
                self.totals.update(tot)
                if over or self.use_hints:  # (the repeat of a step runs without estimates: it keeps the record of what was outgrown)
                    self.last_overflow = over
                if over or outgrown:
                    raise ops.NeighborCapacityExceeded("a neighbour list outgrew its estimated capacity; repeat the step")
        return False

    @staticmethod
    def _key(t):
        return (t.data_ptr(), tuple(t.shape), t._version)

    def _max_count_slot(self, device):
        """One element of a tensor zeroed once per step: where a padded search leaves its longest row (a fill per search otherwise)."""
        pool = getattr(self, "_maxc", None)
        if pool is None or pool[1] >= pool[0].shape[0] or pool[0].device != device:
            pool = self._maxc = [torch.zeros(64, dtype=torch.int32, device=device), 0]
        pool[1] += 1
        return pool[0][pool[1] - 1: pool[1]]

    def _flush(self):
        for r in self.done:
            r.release()
        self.done = []

    def _consumer(self, key, res):
        """Count one consumer of the list; after the last one expected the list leaves the cache and its buffers are dropped
        at the next request (by then the consumer -- layers run one after the other -- has enqueued its kernel)."""
        slot = self.slot_of[key]
        self.uses[slot] = self.uses.get(slot, 0) + 1
        if self.expect.get(slot) == self.uses[slot]:
            self.lists.pop(key, None)
            self.done.append(res)

    def scatter_plan(self, inp_positions, out_positions, voxel, radius, block_cells):
        """dmcf_cconv_scatter_plan for this pair of point sets, once per step."""
        key = (self._key(inp_positions), self._key(out_positions), float(radius), int(block_cells))
        plan = self.plans.get(key) if self.depth > 0 else None
        if plan is None:
            plan = ops.scatter_plan(inp_positions, out_positions, voxel, radius, block_cells)
            if self.depth > 0:
                self.plans[key] = plan
        return plan

    def with_query_points(self, frs, points, queries, radius):
        """For a search that ignores the query points (``frs.ignore_query_point``) over points == queries: the list of the
        SAME search with them, if this step already holds one without distances -- the caller's kernel then skips the pairs
        (i, i) itself (DMCF_FLAG_SKIP_SELF) and the second search of the same point set is not run (the ASCC head after the
        trunk's same-scale layers).  Counts as a consumer of that list.  None when there is nothing to share."""
        if self.depth == 0 or not frs.ignore_query_point:
            return None
        points = points.contiguous()
        queries = queries.contiguous()
        if self._key(points) != self._key(queries):
            return None
        key = ((self._key(points), float(radius)), self._key(queries), False, False)
        hit = self.lists.get(key)
        if hit is not None:
            self._flush()
            self._consumer(key, hit)
        return hit

    def search(self, frs, points, queries, radius, distances=True):
        """``distances=False``: the caller evaluates its window in the kernel, which re-forms d^2 from the positions
        (dmcf_hip.h, neighbors_value == NULL) -- inside a step the list then carries no distance array: half the bytes the
        search writes, half the memory of the list."""
        if self.depth == 0:
            return frs(points, queries, radius)
        if not distances and frs.return_distances:
            frs = frs.index_only()
        self._flush()
        points = points.contiguous()
        queries = queries.contiguous()
        tkey = (self._key(points), float(radius))
        key = (tkey, self._key(queries), frs.ignore_query_point, frs.return_distances)
        hit = self.lists.get(key)
        if hit is not None:
            self._consumer(key, hit)
            return hit
        table = self.tables.get(tkey)
        if table is None or table.n_queries_capacity < queries.shape[0]:
            table = ops.build_spatial_hash_table(points, radius, n_queries=max(points.shape[0], queries.shape[0]))
            self.tables[tkey] = table
        hkey = _hint_key(frs, points, queries, radius)
        # what the estimates of a list are filed under -- who consumes it, how big its buffer was -- is what the search IS
        # (its class) plus, for searches of one class within a step, their order among themselves: a layer that switches
        # between the lattice form and a neighbour list mid-rollout then shifts nobody else's entry (as position in the
        # step's whole search sequence did)
        nth = self.nth.get(hkey, 0)
        self.nth[hkey] = nth + 1
        slot = (hkey, nth)
        hint = self.hints.get(hkey) if self.use_hints else None
        # (A class the previous step did not search -- a new layer form, or the same search whose point sets drifted across a size
        # class boundary -- runs the exact two-pass search once.  Borrowing the stride and pair count of a search one class
        # away was tried in two forms (the largest of the candidates; a unique candidate only): it saves that step's host round
        # trip -- 0.2 ms per step of the 1M bench window, where the lattices grow through the classes -- but the borrowed sizes
        # are fresh block sizes for the allocator: the dam break went from 0 to 2 - 12 device mallocs per rollout.)
        if hint is not None:
            # Padded rows of row_stride(longest row of the previous step) entries: ONE candidate scan per query, no
            # count pass, no prefix scan, no host round trip (HBM is plentiful: 288 GB).  A row that outgrows the
            # stride is detected at the end of the step (one sync) and the step is repeated with the exact search.
            stride, total = row_stride(hint), self.totals.get(slot)
            if total is not None and queries.shape[0] * stride > 4 * total + (1 << 22):
                # ... unless the padded rows would be mostly air: a scene that has dissolved into spray (the 100k dam break
                # after ~40 steps: three times as many lattice points as at the start, most of them around single droplets,
                # next to a bulk whose rows still hold 2,700 entries) took 6 GB per list and 34 GB per step that way.  Then
                # count + scan + write into a buffer sized from the previous step's pairs -- still no host round trip.
                res = frs(points, queries, radius, hash_table=table, capacity_hint=total + total // 4)
            else:
                res = frs(points, queries, radius, hash_table=table, row_stride=stride, capacity_hint=self.caps.get(slot),
                          max_count=self._max_count_slot(points.device))
                self.caps[slot] = getattr(res, "capacity", None)
        else:
            res = frs(points, queries, radius, hash_table=table)
        self.pending.append((hkey, slot, res))
        self.lists[key] = res
        self.slot_of[key] = slot
        self._consumer(key, res)
        self.keepalive.append((points, queries))  # keep storage alive so data_ptr keys stay unique
        return res


class _PerThreadCache:
    """One _NeighborCache per thread: the virtual ranks of dmcf_amd.parallel.run_local_ranks are threads of one process and
    each must see its own step scope, search order and estimates (a real rank is a process and has one anyway)."""

    def __init__(self):
        object.__setattr__(self, "_tls", threading.local())

    def _get(self):
        c = getattr(self._tls, "cache", None)
        if c is None:
            c = self._tls.cache = _NeighborCache()
        return c

    def __getattr__(self, name):
        return getattr(self._get(), name)

    def __setattr__(self, name, value):
        setattr(self._get(), name, value)

    def __enter__(self):
        return self._get().__enter__()

    def __exit__(self, *exc):
        return self._get().__exit__(*exc)


_CACHE = _PerThreadCache()

class _CacheScope:
    """``with neighbor_cache(estimate=...)``: enters the process-wide cache; ``estimate`` (outermost scope only)
    turns on buffer sizes estimated from the previous step -- the caller must then be prepared to repeat the step
    on :class:`dmcf_amd.ops.NeighborCapacityExceeded` (Simulator.run_inference does)."""

    def __init__(self, estimate, key=None):
        self.estimate = estimate
        self.key = key

    def __enter__(self):
        if _CACHE.depth == 0:
            self.prev = _CACHE.use_hints
            _CACHE.use_hints = bool(self.estimate) and os.environ.get("DMCF_NO_ESTIMATE") != "1"
            _CACHE._get().select(self.key)
            self.outer = True
        else:
            self.outer = False
        return _CACHE.__enter__()

    def __exit__(self, *exc):
        try:
            return _CACHE.__exit__(*exc)
        finally:
            if self.outer:
                _CACHE.use_hints = self.prev


def neighbor_cache(estimate=False, key=None):
    """Context manager enabling per-step neighbour-list reuse (see :class:`_NeighborCache`).  ``key``: whose step this is
    -- e.g. (model, scene slot) -- so that the estimates one rollout leaves behind (row capacities, consumers per list, by
    position in the step's search sequence) are not applied to another model or another scene of the same batch."""
    return _CacheScope(estimate, key)


def pairs_ref(nns):
    """The list's pair count as a device scalar -- for the per-launch records of an installed ops.timer only.  Forming it is a
    reduction launch per list (ten per step of a 2-D model, 6 % of its dispatches); a step without a timer never asks: the layers'
    `_avg_neighbors` statistic (convolutions.py:385-388) resolves the list lazily, when somebody reads it."""
    return nns.total_ref if ops.timer is not None else None


def _scatter_guard(vals):
    if any(vals):
        raise RuntimeError("dmcf_cconv_scatter_forward dropped pairs: a block's box did not hold an output it reaches (plan / positions mismatch)")
    return False


def _hint_key(frs, points, queries, radius):
    """What a search is, for the estimates carried from one step to the next: radius, the size class of both point sets
    (half powers of two: particle counts drift by a few per cent per step, the lattices' with them) and the search's flags."""
    def size_class(n):
        return int(round(2.0 * math.log2(max(int(n), 1))))
    return (float(radius), size_class(points.shape[0]), size_class(queries.shape[0]), bool(frs.ignore_query_point),
            bool(frs.return_distances))


class _HintView:
    """The longest-row estimates as a sequence of numbers (tests / diagnostics); ``clear()`` forgets them."""

    def __init__(self, hints):
        self._hints = hints

    def __iter__(self):
        return iter(list(self._hints.values()))

    def __len__(self):
        return len(self._hints)

    def clear(self):
        self._hints.clear()


def neighbor_hints():
    """The longest-row estimates of the process-wide cache (tests / diagnostics)."""
    return _HintView(_CACHE.hints)


def row_stride(longest):
    """Row capacity for the padded single-pass search from the longest row of the previous step: 1/4 slack for long rows; short
    rows get MORE room -- twice the longest row up to 64 entries, + 64 beyond -- because there the maximum over a million rows is
    a noisy statistic (a splash that lands on a wall takes the longest s0 -> s0 row of the 100k dam break from ~35 to ~60 in one
    step: round 3's only repeated step of that 200-step rollout) and room is free: a row's unused tail is neither written nor
    read, and a 1.1M-row list of 80 instead of 56 entries is 110 MB more of 288 GB.  Rounded up to 1/8 of the enclosing power
    of two (a handful of distinct buffer sizes for the caching allocator)."""
    longest = int(longest)
    x = longest + max(longest // 4, min(longest, 64)) + 8
    g = max(8, 1 << max(x.bit_length() - 4, 0))  # 1/8 of the enclosing power of two
    return (x + g - 1) // g * g


def _init_tensor(name, shape, device):
    """Keras initializer strings used by the reference: 'uniform' = RandomUniform(-0.05, 0.05)
    (convolutions.py:156), 'zeros' (:157), 'glorot_uniform' (:169)."""
    if callable(name):
        return name(shape).to(device)
    if name == "uniform":
        return torch.empty(shape, device=device).uniform_(-0.05, 0.05)
    if name == "zeros":
        return torch.zeros(shape, device=device)
    if name == "glorot_uniform":
        fan_in, fan_out = shape[-2] * int(np.prod(shape[:-2])), shape[-1] * int(np.prod(shape[:-2]))
        limit = math.sqrt(6.0 / (fan_in + fan_out))
        return torch.empty(shape, device=device).uniform_(-limit, limit)
    raise NotImplementedError(f"initializer {name!r}")


_ACTIVATIONS = {None: None, "linear": None, "relu": torch.relu, "tanh": torch.tanh}


def _rank1_extents(extents, out_positions):
    """Do these extents take the per-point branch (convolutions.py:366-370, 1006-1010)?  Rank 1 with more than one value, or
    with one per output point; a one-element vector for several outputs stays the scalar it always was here."""
    return (isinstance(extents, torch.Tensor) and extents.dim() == 1
            and (extents.numel() > 1 or extents.numel() == out_positions.shape[0]))


# What the layers prepare for ops.cconv_forward, whichever route a call takes.  A neighbour list with its window is always the
# same six operands: (neighbors_index, neighbors_row_splits, neighbors_row_count, window, window_fac, neighbors_value).

def _scalar_extent(extents, cited):
    """A scalar extent as a Python float; ``cited``: the lines of the reference's class that the refusal names."""
    if isinstance(extents, torch.Tensor):
        if extents.dim() > 0 and extents.numel() != 1:
            raise NotImplementedError(f"extents must be a scalar or of rank 1, [n_out] (convolutions.py:{cited})")
        return float(extents)
    return float(np.float32(extents))


def _search_radius(extent):
    """extent / 2 in float32 arithmetic (:353, :997)."""
    return float(np.float32(0.5) * np.float32(extent))


def _callers_list(user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance):
    """The six operands of the caller's own neighbour list (:341-349, :984-993); None if the caller gave none."""
    if user_neighbors_index is None or user_neighbors_row_splits is None:
        return None
    if user_neighbors_importance is not None and user_neighbors_importance.numel() > 0:
        return user_neighbors_index, user_neighbors_row_splits, None, "explicit", 1.0, user_neighbors_importance
    return user_neighbors_index, user_neighbors_row_splits, None, None, 1.0, None


def _window_operands(window_function, nns, radius):
    """The six operands of a FixedRadiusSearch result at ``radius`` (:359-379, :1015-1019)."""
    # raw(): buffers that may be longer than P (no host round trip); the kernels only follow row_splits
    neighbors_index, neighbors_row_splits, raw_dist = nns.raw()
    row_count = getattr(nns, "row_count", None)  # padded rows of the single-pass search
    if window_function is None:
        return neighbors_index, neighbors_row_splits, row_count, None, 1.0, None
    if isinstance(window_function, WindowFunction):
        # d^2; q = d^2/R^2 is formed in the kernel
        return neighbors_index, neighbors_row_splits, row_count, window_function.name, window_function.fac, raw_dist
    q = nns.neighbors_distance / (np.float32(radius) * np.float32(radius))
    neighbors_index = nns.neighbors_index  # compact CSR form (synchronises)
    if row_count is not None:
        neighbors_row_splits, row_count = nns.csr_row_splits, None
    return neighbors_index, neighbors_row_splits, row_count, "explicit", 1.0, window_function(q).to(torch.float32)


def _extents_lists(layer, inp_positions, out_positions, extents, user_neighbors_index, user_neighbors_row_splits,
                   user_neighbors_importance):
    """The six operands of the rank-1 branch, for ContinuousConv (inference and recording) and PointSampling alike: the
    caller's list, or a RadiusSearch at radii = extents / 2 (:366-370, :1006-1010; kept in ``layer.nns``).  Call under no_grad."""
    n_out = out_positions.shape[0]
    if extents.shape[0] != n_out:
        raise ValueError(f"extents of rank 1 must hold one value per output point ({n_out}), got {extents.shape[0]}")
    lists = _callers_list(user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance)
    if lists is not None:
        return lists
    named = isinstance(layer.window_function, WindowFunction)
    # (a named window is evaluated in the kernel on d^2 re-formed from the positions: no distances needed)
    search = layer.radius_search.index_only() if named else layer.radius_search
    layer.__dict__["nns"] = search(inp_positions, out_positions, 0.5 * extents)  # :367
    neighbors_index, neighbors_row_splits, dist = layer.nns
    window, window_fac, neighbors_value = None, 1.0, None
    if layer.window_function is not None:
        # The reference's rank-1 branch never binds neighbors_distance_normalized (:366-379: only the rank-0 branch
        # does), so with a window TensorFlow raises there.  Implemented is the evident intent: the window on the
        # RadiusSearch distances normalised per query, d^2 / r_i^2 (its normalize_distances=True, :212-216).
        if named:
            window, window_fac = layer.window_function.name, layer.window_function.fac  # q = d^2 / r_i^2 in the kernel
        else:
            window, neighbors_value = "explicit", layer.window_function(dist).to(torch.float32)
    return neighbors_index, neighbors_row_splits, None, window, window_fac, neighbors_value


class PlainAttributes:
    """Mix-in for the modules of this package: attributes that are neither parameters, buffers nor sub-modules go straight to the
    instance dictionary.  torch.nn.Module.__setattr__ walks its registries and type checks for every assignment -- a layer sets
    a dozen bookkeeping attributes per call (the reference's ``.nns``, ``._conv_values``, ...), 300 assignments per step of a 2-D
    model: a fifth of that step's host time (tools/profile_small.py)."""

    def __setattr__(self, name, value):
        d = self.__dict__
        if (isinstance(value, (torch.nn.Parameter, torch.nn.Module)) or "_parameters" not in d or name in d["_parameters"]
                or name in d["_buffers"] or name in d["_modules"] or hasattr(type(self), name)):
            super().__setattr__(name, value)  # (registries; properties and other class-level descriptors keep their setters)
        else:
            d[name] = value


class ContinuousConv(PlainAttributes, torch.nn.Module):
    r"""Continuous convolution of Ummenhofer & Koltun (ICLR 2020) with DMCF's antisymmetric option:

        (f*g)(x) = 1/psi(x) * sum_{i in N(x,R)} a(x_i, x) f_i g(Lambda(x_i - x))

    Arguments are those of the reference layer (utils/convolutions.py:67-149).  Unsupported
    combinations raise instead of silently computing something else.
    """

    def __init__(self, filters, kernel_size, activation=None, use_bias=True, kernel_initializer="uniform",
                 bias_initializer="zeros", kernel_regularizer=None, bias_regularizer=None, align_corners=True,
                 coordinate_mapping="ball_to_cube_radial", interpolation="linear", normalize=True,
                 radius_search_ignore_query_points=False, radius_search_metric="L2", offset=None,
                 window_function=None, use_dense_layer_for_center=False,
                 dense_kernel_initializer="glorot_uniform", dense_kernel_regularizer=None, in_channels=None,
                 symmetric=False, sym_axis=2, circular=False, name=None, trainable=True, device=None,
                 record_per_point_extents=False, record_lattice_form=False, record_scatter_form=False, **kwargs):
        super().__init__()
        self.layer_name = name
        # may a call with extents of rank 1 record autograd history (_forward_train; not a keyword of the reference)
        self.record_per_point_extents = bool(record_per_point_extents)
        # may a recording call between two grid_pos lattices keep the stencil form (_forward_train; dmcf_lattice_conv_backward)
        self.record_lattice_form = bool(record_lattice_form)
        # may a recording call from particles onto a grid_pos lattice with 4 or 8 output channels take the input-stationary
        # backward on the transposed list (_forward_train; dmcf_cconv_scatter_backward)
        self.record_scatter_form = bool(record_scatter_form)
        self.filters = filters
        self.kernel_size = [int(k) for k in kernel_size]
        if activation not in _ACTIVATIONS and not callable(activation):
            raise NotImplementedError(f"activation {activation!r}")
        self.activation = _ACTIVATIONS.get(activation, activation) if not callable(activation) else activation
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.align_corners = align_corners
        if coordinate_mapping not in ops.MAPPINGS:
            raise ValueError(f"coordinate_mapping {coordinate_mapping!r}")
        if interpolation not in ops.INTERPOLATIONS:
            raise ValueError(f"interpolation {interpolation!r}")
        self.coordinate_mapping = coordinate_mapping
        self.interpolation = interpolation
        self.normalize = normalize
        self.radius_search_ignore_query_points = radius_search_ignore_query_points
        self.radius_search_metric = radius_search_metric
        self.dense_kernel_initializer = dense_kernel_initializer
        self.symmetric = symmetric
        self.sym_axis = sym_axis
        self.circular = circular
        if offset is not None and any(float(o) != 0.0 for o in torch.as_tensor(offset).reshape(-1)):
            raise NotImplementedError("non-zero offset (never used by DMCF, convolutions.py:200-201)")
        self.offset = torch.zeros(3)
        self.window_function = window_function
        # convolutions.py:207-210
        self.fixed_radius_search = ops.FixedRadiusSearch(
            metric=self.radius_search_metric, ignore_query_point=self.radius_search_ignore_query_points,
            return_distances=self.window_function is not None)
        # convolutions.py:212-216 (extents of rank 1)
        self.radius_search = ops.RadiusSearch(
            metric=self.radius_search_metric, ignore_query_point=self.radius_search_ignore_query_points,
            return_distances=self.window_function is not None, normalize_distances=self.window_function is not None)
        self.use_dense_layer_for_center = use_dense_layer_for_center
        self.dense = None
        self.in_channels = None
        self.kernel = None
        self.bias = None
        self._device = device
        self.nns = None
        self._direct_kernel = None  # is this layer served by cconv_direct_kernel (learnt at its first call in a step)
        # what the MODEL knows about this layer's rows from its configuration (include/dmcf_hip.h, row_length_hint): 0 unknown,
        # 1 = the network's base radius (tens of neighbours), 2 = a wider radius (hundreds); models/hrnet.py sets it
        self.row_length_hint = 0
        self.accumulate_into = None  # one-shot, see forward
        self.extra_bias = None
        self._packed = {}  # the workspace of the last dmcf_cconv_forward and what its packed filter was made from (ops.cconv_forward)

    def invalidate_packed(self):
        """Drops the cached packed filter (ops.cconv_forward).  Needed only after writing the weights through ``.data`` --
        the one way to change a tensor that its version counter does not see."""
        self._packed.clear()

    def _load_from_state_dict(self, *args, **kwargs):
        self._packed.clear()
        return super()._load_from_state_dict(*args, **kwargs)

    # -- weights (lazy, from the first input's channel count: convolutions.py:228-275) ----------------
    def build(self, in_channels, device=None):
        self._packed.clear()
        device = device or self._device or "cuda"
        self.in_channels = int(in_channels)
        if self.circular:
            kshape = (math.ceil(max(self.kernel_size) / 2), self.in_channels, self.filters)  # :231-234
        elif self.symmetric:
            sh = list(self.kernel_size)
            assert sh[self.sym_axis] % 2 == 0  # :244
            sh[self.sym_axis] = sh[self.sym_axis] // 2
            kshape = (*sh, self.in_channels, self.filters)
        else:
            kshape = (*self.kernel_size, self.in_channels, self.filters)
        self.kernel = torch.nn.Parameter(_init_tensor(self.kernel_initializer, kshape, device), requires_grad=False)
        if self.use_bias:
            self.bias = torch.nn.Parameter(_init_tensor(self.bias_initializer, (self.filters,), device),
                                           requires_grad=False)
        if self.use_dense_layer_for_center:
            w = _init_tensor(self.dense_kernel_initializer, (self.in_channels, self.filters), device)
            self.dense = torch.nn.Parameter(w, requires_grad=False)

    def _expanded_kernel(self):
        """circular kernels (convolutions.py:395-409): ring index = max_axis floor(|grid offset|)."""
        ks = self.kernel_size
        zr, yr, xr = torch.meshgrid(*[torch.arange(k, device=self.kernel.device) for k in ks], indexing="ij")
        size_xyz = torch.tensor(ks[::-1], dtype=torch.float32, device=self.kernel.device)
        gp = torch.stack([xr, yr, zr], dim=-1).to(torch.float32) - size_xyz / 2.0 + 0.5
        mask = (gp * 2.0) / size_xyz
        idx = torch.floor(gp.abs()).max(dim=-1).values.to(torch.int64)
        kernel = self.kernel[idx]
        if self.symmetric:
            # NOTE: the reference multiplies by mask[..., None, :] (shape [D,H,W,1,3]), which only
            # broadcasts when filters == 3 (convolutions.py:408-409)
            kernel = kernel * mask.unsqueeze(-2)
        return kernel

    def forward(self, inp_features, inp_positions, out_positions, extents, inp_importance=None,
                fixed_radius_search_hash_table=None, user_neighbors_index=None, user_neighbors_row_splits=None,
                user_neighbors_importance=None, inp_positions_row_splits=None, out_positions_row_splits=None):
        """The reference's arguments, and after them ``inp_positions_row_splits`` / ``out_positions_row_splits`` (both or
        neither): a BATCH of point sets in one call -- item b is inp_positions[irs[b]:irs[b+1]] and
        out_positions[ors[b]:ors[b+1]], an output point gathers from input points of its own item only (see _batched_lists)."""
        if inp_positions_row_splits is not None or out_positions_row_splits is not None:
            user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance = self._batched_lists(
                inp_positions, out_positions, extents, inp_positions_row_splits, out_positions_row_splits,
                user_neighbors_index, user_neighbors_row_splits, fixed_radius_search_hash_table)
        if self.kernel is None:
            with torch.no_grad():
                self.build(inp_features.shape[-1], inp_features.device)
        if self.recording(inp_features):
            return self._forward_train(inp_features, inp_positions, out_positions, extents, inp_importance,
                                       fixed_radius_search_hash_table, user_neighbors_index, user_neighbors_row_splits,
                                       user_neighbors_importance)
        return self._forward_infer(inp_features, inp_positions, out_positions, extents, inp_importance,
                                   fixed_radius_search_hash_table, user_neighbors_index, user_neighbors_row_splits,
                                   user_neighbors_importance)

    @torch.no_grad()
    def _batched_lists(self, inp_positions, out_positions, extents, inp_row_splits, out_row_splits, user_neighbors_index,
                       user_neighbors_row_splits, hash_table=None):
        """The neighbour list of a batched call, handed to the layer's user-list path (:341-349): (neighbors_index,
        neighbors_row_splits, neighbors_importance).  The batched search -- FixedRadiusSearch at 0.5 * extent for a scalar
        extent, RadiusSearch at 0.5 * extents for extents of rank 1 -- then the layer's window function on the normalised
        distances d^2 / r^2 as the importance (None without a window).  The list is an arbitrary CSR list over the
        concatenated points, which every neighbour-list kernel takes, forward and backward; the lattice, scatter and direct
        forms and the step's list cache do not apply."""
        if inp_row_splits is None or out_row_splits is None:
            raise NotImplementedError("a batched call needs both inp_positions_row_splits and out_positions_row_splits")
        if user_neighbors_index is not None or user_neighbors_row_splits is not None:
            raise ValueError("row splits and a user neighbour list exclude each other: the list already says who is whose neighbour")
        if self.symmetric:
            raise NotImplementedError("symmetric=True (ASCC) with row splits is not implemented")
        return self._batched_search(inp_positions, out_positions, extents, inp_row_splits, out_row_splits, hash_table)

    @torch.no_grad()
    def _batched_search(self, inp_positions, out_positions, extents, inp_row_splits, out_row_splits, hash_table=None):
        """The search and the importance of _batched_lists.  ``hash_table``: a batched structure of (inp_positions, 0.5 * extent,
        inp_row_splits) to search in (ops.build_spatial_hash_table with points_row_splits) -- a model's batched step builds
        one per point set and radius and hands it to every layer that reads that set (models/pbf_model.py)."""
        splits = dict(points_row_splits=inp_row_splits, queries_row_splits=out_row_splits)
        if _rank1_extents(extents, out_positions):
            if extents.shape[0] != out_positions.shape[0]:
                raise ValueError(f"extents of rank 1 must hold one value per output point ({out_positions.shape[0]}), "
                                 f"got {extents.shape[0]}")
            nns = self.radius_search(inp_positions, out_positions, 0.5 * extents.detach(), **splits)  # :367, normalised by the search
            q = nns.neighbors_distance
        else:
            radius = _search_radius(_scalar_extent(extents, "352-372"))
            if hash_table is not None:
                splits["hash_table"] = hash_table
            nns = self.fixed_radius_search(inp_positions, out_positions, radius, **splits)
            q = nns.neighbors_distance / (np.float32(radius) * np.float32(radius)) if self.window_function is not None else None
        self.__dict__["nns"] = nns
        importance = None if self.window_function is None else self.window_function(q).to(torch.float32)
        return nns.neighbors_index, nns.neighbors_row_splits, importance

    def recording(self, inp_features=None):
        """Does a call now record autograd history: grad mode on and a weight (``requires_grad_(True)``) or the input features
        requiring grad.  Weights are built with requires_grad=False, so inference never records."""
        if not torch.is_grad_enabled():
            return False
        if isinstance(inp_features, torch.Tensor) and inp_features.requires_grad:
            return True
        return any(w is not None and w.requires_grad for w in (self.kernel, self.bias, self.dense))

    def _forward_train(self, inp_features, inp_positions, out_positions, extents, inp_importance, hash_table,
                       user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance):
        """The layer while autograd records: the neighbour-list form through ops.cconv_forward's autograd node
        (dmcf_cconv_backward; extents of rank 1, one per output point, in a layer built with record_per_point_extents=True:
        dmcf_cconv_backward_extents).  A layer built with record_lattice_form=True keeps the stencil form between two grid_pos
        lattices (ops.lattice_conv's autograd node, dmcf_lattice_conv_backward: no search, no inversion) when the pair is whole --
        no stray rows -- and its spacings are in the ratio 1, 2 or 1/2; opt-in, because that form uses the nominal offsets
        d * voxel (dmcf_amd/lattice.py) where the neighbour-list form subtracts rounded positions.  A layer built with
        record_scatter_form=True that gathers particles onto a grid_pos lattice with 4 or 8 output channels (_scatter_train_form;
        scalar extent, no user-supplied list) takes ops.ScatterConvFunction: its backward is one dmcf_cconv_scatter_backward over
        the transposed list, which a search with the roles swapped returns -- no inversion; its forward is the scatter form where
        inference would take it (_scatter_form), otherwise the neighbour-list form on the layer's own forward list.  A layer with
        either flag that is not eligible takes the neighbour-list route and gives the bits it gives with the flag off.  The
        stray-row path, the step's list cache and the epilogue fusions
        (accumulate_into / extra_bias, fused bias) are not taken: their kernels have no backward.  Bias, the dense centre term,
        the activation and the circular expansion are torch ops.  A pending accumulate_into / extra_bias request is honoured out
        of place: the result is ``accumulate_into + layer(x) + extra_bias`` (accumulate_into itself is not written)."""
        d = self.__dict__
        acc, extra_bias = self.accumulate_into, self.extra_bias
        d["accumulate_into"] = d["extra_bias"] = None
        users = (user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance)
        rank1 = _rank1_extents(extents, out_positions)
        if rank1 and not self.record_per_point_extents:
            raise NotImplementedError("ContinuousConv with per-point extents (rank 1) records only when built with "
                                      "record_per_point_extents=True; without it the training path takes a scalar extent only")
        if rank1:
            # one extent per output point (:366-370): the search and the window of _forward_extents, then the same call -- the
            # extents go to ops.cconv_forward as a tensor and get no gradient, as in Open3D
            with torch.no_grad():
                extent = extents.detach()
                lists = _extents_lists(self, inp_positions, out_positions, extent, *users)
        else:
            extent = _scalar_extent(extents, "352-372")
        lat = None
        if self.record_lattice_form and not rank1 and (user_neighbors_index is None or user_neighbors_row_splits is None):
            lat = self._lattice_form(inp_features, inp_positions, out_positions, inp_importance, hash_table, extent)
            if lat is not None and (lat.cropped or lat.ratio not in (1, 2, 0.5)):
                lat = None  # (stray rows would need the neighbour-list form beside it: the whole layer takes that form)
        if lat is not None:
            d["nns"] = None
            d["_n_out_last"] = out_positions.shape[0]
            d["_pairs_last"] = 0
            d["_conv_values"] = None
            out_features = lat.conv(ops, self.kernel, inp_features, out_positions.shape[0], extent,
                                    window=self.window_function.name, window_fac=self.window_function.fac, **self._geometry())
            return self._train_epilogue(out_features, inp_features, acc, extra_bias)
        if (self.record_scatter_form and not rank1 and user_neighbors_index is None and user_neighbors_row_splits is None
                and self._scatter_train_form(inp_features, inp_positions, out_positions, inp_importance, hash_table)):
            out_features = self._scatter_train(inp_features, inp_positions, out_positions, extent)
            return self._train_epilogue(out_features, inp_features, acc, extra_bias)
        if not rank1:
            lists = _callers_list(*users)
            if lists is None:
                radius = _search_radius(extent)
                with torch.no_grad():
                    # (an exact search of its own, outside the step's list cache: the backward needs the list after the step)
                    d["nns"] = self.fixed_radius_search(inp_positions, out_positions, radius, hash_table=hash_table)
                    lists = _window_operands(self.window_function, self.nns, radius)
        neighbors_index, neighbors_row_splits, row_count, window, window_fac, neighbors_value = lists
        d["_n_out_last"] = out_positions.shape[0]
        d["_pairs_last"] = neighbors_index.shape[0]
        kernel, symmetric = self._conv_kernel()
        d["_conv_values"] = None
        out_features = ops.cconv_forward(
            kernel, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
            neighbors_value=neighbors_value, window=window, window_fac=window_fac, inp_importance=inp_importance,
            neighbors_row_count=row_count, row_length_hint=self.row_length_hint, packed_cache=self._packed_cache(kernel),
            **self._geometry(symmetric), **({"record_per_point_extents": True} if rank1 else {}))
        return self._train_epilogue(out_features, inp_features, acc, extra_bias)

    def _scatter_train(self, inp_features, inp_positions, out_positions, extent):
        """The convolution (no bias) of a recording call on the record_scatter_form route: ops.ScatterConvFunction over the
        transposed list of an exact search with the roles swapped (the neighbour set is symmetric, so the list holds the forward's
        pairs).  The forward inside the node is what inference computes for these operands."""
        d = self.__dict__
        radius = _search_radius(extent)
        window, window_fac = self.window_function.name, self.window_function.fac
        with torch.no_grad():
            # (a search of its own, outside the step's list cache: the backward needs the list after the step)
            tl = ops.fixed_radius_search(out_positions, inp_positions, radius, return_distances=False)
            t_idx, t_rb, _ = tl.raw()
            t_cnt = getattr(tl, "row_count", None)
            sct = self._scatter_form(inp_features, inp_positions, out_positions, None, None, radius)
        d["nns"] = None
        d["_n_out_last"] = out_positions.shape[0]
        d["_pairs_last"] = t_idx.shape[0]
        d["_conv_values"] = None
        geo = dict(extent=extent, window=window, window_fac=window_fac)
        if sct is not None:
            voxel, m = sct

            def run(w, f, **lists):
                flag = torch.zeros(1, dtype=torch.int32, device=inp_positions.device)
                out = ops.cconv_scatter_forward(w, inp_features=f, plan=_CACHE.scatter_plan(inp_positions, out_positions, voxel, radius, m),
                                                error_flag=flag, **lists, **geo)
                _CACHE.report(flag, _scatter_guard)
                return out
        else:
            def run(w, f, **lists):
                nns = self.fixed_radius_search(inp_positions, out_positions, radius)
                idx, rs, raw_dist = nns.raw()
                return ops.cconv_forward(w, out_positions, extent, inp_positions, f, idx, rs, neighbors_value=raw_dist, window=window,
                                         window_fac=window_fac, neighbors_row_count=getattr(nns, "row_count", None),
                                         row_length_hint=self.row_length_hint, **self._geometry())
        return ops.ScatterConvFunction.apply(self.kernel, inp_features, out_positions, inp_positions, t_idx, t_rb, t_cnt, geo, run)

    def _train_epilogue(self, out_features, inp_features, acc, extra_bias):
        """What follows the convolution of a recording call, as torch ops: bias, dense centre term, activation, the sums."""
        if self.use_bias and not self.use_dense_layer_for_center:
            out_features = out_features + self.bias
        self.__dict__["_conv_output"] = None
        # (where the inference path puts the extra bias: inside the activation, unless the call also accumulates)
        out_features = self._finish(out_features, inp_features, extra_bias if acc is None else None)
        if acc is not None:
            out_features = acc + out_features
            if extra_bias is not None:
                out_features = out_features + extra_bias
        return out_features

    @torch.no_grad()
    def _forward_infer(self, inp_features, inp_positions, out_positions, extents, inp_importance=None,
                       fixed_radius_search_hash_table=None, user_neighbors_index=None, user_neighbors_row_splits=None,
                       user_neighbors_importance=None):
        # one-shot requests of the caller (models/hrnet.py): add the result to this tensor in the kernel's epilogue
        # (DMCF_FLAG_ACCUMULATE) instead of returning a new one, and add this vector to the layer's bias
        acc, extra_bias = self.accumulate_into, self.extra_bias
        d = self.__dict__  # (bookkeeping attributes written straight to the instance dictionary: PlainAttributes would put them there too)
        d["accumulate_into"] = d["extra_bias"] = None
        if acc is not None and (self.use_dense_layer_for_center or self.activation is not None or not acc.is_contiguous()
                                or tuple(acc.shape) != (out_positions.shape[0], self.filters) or acc.dtype != torch.float32):
            # not expressible in the epilogue: the plain call, then the sums (the extra bias OUTSIDE the layer's activation)
            acc.add_(self.forward(inp_features, inp_positions, out_positions, extents, inp_importance,
                                  fixed_radius_search_hash_table, user_neighbors_index, user_neighbors_row_splits,
                                  user_neighbors_importance))
            return acc if extra_bias is None else acc.add_(extra_bias)
        if _rank1_extents(extents, out_positions):
            return self._forward_extents(inp_features, inp_positions, out_positions, extents, inp_importance, user_neighbors_index,
                                         user_neighbors_row_splits, user_neighbors_importance, acc, extra_bias)
        extent = _scalar_extent(extents, "352-372")
        n_pairs_ref, skip_self = None, False
        lists = _callers_list(user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance)
        if lists is None:
            lat = self._lattice_form(inp_features, inp_positions, out_positions, inp_importance,
                                     fixed_radius_search_hash_table, extent)
            if lat is not None:
                # both point sets are grid_pos lattices of this step: no search, no per-pair geometry
                # (dmcf_lattice_conv_forward; DMCF_LATTICE_CONV=0 keeps the neighbour-list form)
                d["nns"] = None
                d["_n_out_last"] = out_positions.shape[0]
                d["_pairs_last"] = 0  # no pair list in this form
                out_features = lat.conv(
                    ops, self.kernel, inp_features, out_positions.shape[0], extent,
                    window=self.window_function.name, window_fac=self.window_function.fac, **self._geometry(),
                    bias=self._epilogue_bias(extra_bias), out=acc, accumulate=acc is not None)
                stray = lat.strays()
                if stray is not None:
                    # output points outside the lattice's core (stray particles' cells, dmcf_amd/lattice.py): the same layer
                    # through a neighbour list over ALL input points, added to their rows of the result (rows the stencil form
                    # does not write: zero, or the value to accumulate to).  The row set has an estimated capacity inside a
                    # rollout: ``valid`` zeroes the padding rows
                    idx_s, pos_s, valid = stray
                    nns = _CACHE.search(self.fixed_radius_search, inp_positions, pos_s, _search_radius(extent), distances=False)
                    ni, nrs, raw_dist = nns.raw()
                    # (normalize and symmetric are off wherever this form applies; the rows are short whatever the layer's are)
                    res = ops.cconv_forward(
                        self.kernel, pos_s, extent, inp_positions, inp_features, ni, nrs, neighbors_value=raw_dist,
                        window=self.window_function.name, window_fac=self.window_function.fac, **self._geometry(),
                        bias=self._epilogue_bias(extra_bias), n_pairs_ref=pairs_ref(nns),
                        neighbors_row_count=getattr(nns, "row_count", None), row_length_hint=1)
                    if valid is not None:
                        res = res * valid
                    out_features.index_add_(0, idx_s, res)
                d["_conv_values"], d["_conv_output"] = None, (None if _CACHE.depth > 0 else out_features)
                return self._finish(out_features, inp_features, extra_bias if self.use_dense_layer_for_center else None)
            radius = _search_radius(extent)
            sct = self._scatter_form(inp_features, inp_positions, out_positions, inp_importance, fixed_radius_search_hash_table,
                                     radius)
            if sct is not None:
                # particles -> coarse lattice with 4 output channels: filter first, input stationary, over the TRANSPOSED list
                # (dmcf_cconv_scatter_forward; DMCF_SCATTER_CONV=0 keeps the gather form) -- the list of the later
                # lattice -> particles layers of the step, searched here if this layer is the first to ask for it
                voxel, m = sct
                tl = _CACHE.search(self.fixed_radius_search, out_positions, inp_positions, radius, distances=False)
                t_idx, t_rb, _ = tl.raw()
                d["nns"] = None
                d["_n_out_last"] = out_positions.shape[0]
                d["_pairs_last"] = tl
                # (the kernel's guard -- a pair outside its block's box, i.e. a plan that does not match the positions -- is read with
                # the step's one synchronisation and fails loudly; it has never fired)
                flag = _CACHE._max_count_slot(inp_positions.device) if _CACHE.depth > 0 else torch.zeros(1, dtype=torch.int32, device=inp_positions.device)
                out_features = ops.cconv_scatter_forward(
                    self.kernel, out_positions, extent, inp_positions, inp_features, t_idx, t_rb, getattr(tl, "row_count", None),
                    _CACHE.scatter_plan(inp_positions, out_positions, voxel, radius, m), window=self.window_function.name,
                    window_fac=self.window_function.fac, bias=self._epilogue_bias(extra_bias), out=acc,
                    accumulate=acc is not None, n_pairs_ref=pairs_ref(tl), error_flag=flag)
                _CACHE.report(flag, _scatter_guard)
                d["_conv_values"], d["_conv_output"] = None, (None if _CACHE.depth > 0 else out_features)
                return self._finish(out_features, inp_features, extra_bias if self.use_dense_layer_for_center else None)
            if fixed_radius_search_hash_table is not None:
                d["nns"] = self.fixed_radius_search(inp_positions, out_positions, radius,
                                                    hash_table=fixed_radius_search_hash_table)
            else:
                shared = None
                if self._shares_list():
                    shared = _CACHE.with_query_points(self.fixed_radius_search, inp_positions, out_positions, radius)
                skip_self = shared is not None
                d["nns"] = shared if skip_self else _CACHE.search(
                    self.fixed_radius_search, inp_positions, out_positions, radius,
                    distances=not isinstance(self.window_function, WindowFunction))
            n_pairs_ref = pairs_ref(self.nns)
            lists = _window_operands(self.window_function, self.nns, radius)
        neighbors_index, neighbors_row_splits, row_count, window, window_fac, neighbors_value = lists
        # stats (convolutions.py:385-388) are formed lazily (property _avg_neighbors): no host sync here
        d["_n_out_last"] = out_positions.shape[0]
        d["_pairs_last"] = self.nns if (n_pairs_ref is None and getattr(self, "nns", None) is not None and user_neighbors_index is None) \
            else (n_pairs_ref if n_pairs_ref is not None else neighbors_index.shape[0])

        kernel, symmetric = self._conv_kernel()
        in_step = self._keep_operands(kernel, out_positions, extent, inp_positions, inp_features, inp_importance, neighbors_index,
                                      neighbors_row_splits, neighbors_value)
        # the operands of the launch and of the question which kernel serves it
        operands = dict(neighbors_value=neighbors_value, window=window, window_fac=window_fac, inp_importance=inp_importance,
                        neighbors_row_count=row_count, **self._geometry(symmetric))
        out_features = ops.cconv_forward(
            kernel, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits, **operands,
            bias=self._epilogue_bias(extra_bias), n_pairs_ref=n_pairs_ref, skip_self=skip_self,
            row_length_hint=self.row_length_hint, out=acc, accumulate=acc is not None, packed_cache=self._packed_cache(kernel))
        if self._direct_kernel is None and in_step and self.radius_search_ignore_query_points:
            # (asked once per layer: the dispatch looks at the layer, never at the list)
            self._direct_kernel = ops.cconv_forward(
                kernel, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits, **operands,
                name_only=True).startswith("cconv_direct_kernel")
            if self._shares_list() and user_neighbors_index is None and fixed_radius_search_hash_table is None:
                # announce this layer as one more consumer of the list it will take from the next step on (the cache hands a
                # list's buffers back after the number of consumers it saw in the previous step)
                _CACHE.with_query_points(self.fixed_radius_search, inp_positions, out_positions, _search_radius(extent))
        d["_conv_output"] = None if in_step else out_features
        return self._finish(out_features, inp_features, extra_bias if self.use_dense_layer_for_center else None)

    def _geometry(self, symmetric=None):
        """The layer's fixed options as keywords of ops.cconv_forward.  ``symmetric`` None: the mapping alone -- what the
        lattice form takes, and the list calls beside it (stray rows, the list forward of the scatter route), which run only
        where normalize and symmetric are off."""
        geometry = dict(align_corners=self.align_corners, coordinate_mapping=self.coordinate_mapping, interpolation=self.interpolation)
        if symmetric is not None:
            geometry.update(normalize=self.normalize, symmetric=symmetric, sym_axis=self.sym_axis)
        return geometry

    def _packed_cache(self, kernel):
        """Where ops.cconv_forward keeps the packed filter of this layer (a derived filter tensor -- circular -- is a new object
        every call: never cached)."""
        return self._packed if (kernel is self.kernel and os.environ.get("DMCF_CACHE_PACKED_FILTERS", "1") != "0") else None

    def _keep_operands(self, kernel, out_positions, extents, inp_positions, inp_features, inp_importance, neighbors_index,
                       neighbors_row_splits, neighbors_value):
        """The reference keeps the operands of the last call for inspection (``_conv_values``, convolutions.py:398-413).  Inside a
        rollout step (neighbor_cache scope) that would pin every layer's neighbour list (GBs each) and activations into the
        next step: there only the small entries are kept.  Returns whether the call is inside a step."""
        in_step = _CACHE.depth > 0
        self.__dict__["_conv_values"] = {
            "filters": kernel, "out_positions": out_positions, "extents": extents, "offset": self.offset,
            "inp_positions": inp_positions, "inp_features": None if in_step else inp_features,
            "inp_importance": inp_importance,
            "neighbors_index": None if in_step else neighbors_index, "neighbors_row_splits": neighbors_row_splits,
            "neighbors_importance": None if in_step else neighbors_value, "align_corners": self.align_corners,
            "coordinate_mapping": self.coordinate_mapping, "interpolation": self.interpolation,
            "normalize": self.normalize,
        }
        return in_step

    def _conv_kernel(self):
        """(filter tensor, fused ASCC?) of a call: the circular expansion (convolutions.py:395-409) or the stored kernel."""
        kernel, symmetric = self.kernel, self.symmetric
        if self.circular:
            # (refused before the expansion, whose mask broadcasts only when filters == 3)
            if self.symmetric:
                raise NotImplementedError("circular + symmetric kernels (filters must be 3 in the reference; "
                                          "no shipped config uses circular: True)")
            kernel = self._expanded_kernel()
            symmetric = False  # the mask already made it antisymmetric; second pass still applies below
        if symmetric and self.normalize:
            raise NotImplementedError("symmetric=True with normalize=True (DMCF always uses normalize=False, "
                                      "models/pbf_model.py:203)")
        return kernel, symmetric

    def _forward_extents(self, inp_features, inp_positions, out_positions, extents, inp_importance, user_neighbors_index,
                         user_neighbors_row_splits, user_neighbors_importance, acc, extra_bias):
        """The branch for extents of rank 1 (convolutions.py:366-370, then :397-399): a radius per output point (RadiusSearch),
        every row convolved at its own extent (ops.cconv_forward -> dmcf_cconv_forward_extents; with SYMMETRIC each pair at its
        output row's extent, which does not conserve momentum).  Never the lattice / scatter forms or the step's neighbour
        cache: all of them key on one radius."""
        d = self.__dict__
        n_out = out_positions.shape[0]
        neighbors_index, neighbors_row_splits, _, window, window_fac, neighbors_value = _extents_lists(
            self, inp_positions, out_positions, extents, user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance)
        d["_n_out_last"] = n_out
        d["_pairs_last"] = neighbors_index.shape[0]
        kernel, symmetric = self._conv_kernel()
        in_step = self._keep_operands(kernel, out_positions, extents.reshape(n_out, 1), inp_positions, inp_features, inp_importance,
                                      neighbors_index, neighbors_row_splits, neighbors_value)
        out_features = ops.cconv_forward(
            kernel, out_positions, extents, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
            neighbors_value=neighbors_value, window=window, window_fac=window_fac, inp_importance=inp_importance,
            **self._geometry(symmetric), bias=self._epilogue_bias(extra_bias), out=acc, accumulate=acc is not None)
        d["_conv_output"] = None if in_step else out_features
        return self._finish(out_features, inp_features, extra_bias if self.use_dense_layer_for_center else None)

    def _epilogue_bias(self, extra_bias):
        """The vector the kernel's epilogue adds: the layer's bias + the caller's."""
        if self.use_dense_layer_for_center:
            return None  # (bias and the caller's vector follow the dense term, _finish)
        bias = self.bias if self.use_bias else None
        if extra_bias is None:
            return bias
        return extra_bias if bias is None else bias + extra_bias

    def _shares_list(self):
        """May this layer take the list of the same search WITH the query points (see _NeighborCache.with_query_points)?  Only
        a layer that ignores them, evaluates a named window in the kernel and is served by the kernel that implements
        DMCF_FLAG_SKIP_SELF; DMCF_SHARE_LISTS=0 turns it off."""
        return (self.radius_search_ignore_query_points and self._direct_kernel is True and self.radius_search_metric == "L2"
                and isinstance(self.window_function, WindowFunction) and os.environ.get("DMCF_SHARE_LISTS", "1") != "0")

    def _finish(self, out_features, inp_features, extra_bias=None):
        if self.use_dense_layer_for_center:  # :462-464
            dense_output = inp_features @ self.dense
            self._dense_output = None if _CACHE.depth > 0 else dense_output
            out_features = out_features + dense_output
            if self.use_bias:
                out_features = out_features + self.bias
        if extra_bias is not None:
            out_features = out_features + extra_bias
        if self.activation is not None:
            out_features = self.activation(out_features)
        return out_features

    def _scatter_lattice(self, inp_features, out_positions, inp_importance, hash_table):
        """The output lattice if the input-stationary kernels (dmcf_cconv_scatter_forward / _backward) implement this call, else
        None: the outputs are a registered grid_pos lattice with one spacing on all axes, a filter of a shape the library takes
        (ops.cconv_scatter_supported, asked with the smallest box) with the options those kernels implement, and the default
        (symmetric) neighbour set -- the transposed list then holds the same pairs as the forward one."""
        from .. import lattice
        if (not lattice.enabled() or hash_table is not None
                or inp_importance is not None or self.symmetric or self.circular or self.normalize
                or not isinstance(self.window_function, WindowFunction) or self.window_function.name != "poly6"
                or self.radius_search_ignore_query_points or self.radius_search_metric != "L2" or not inp_features.is_cuda
                or not self.align_corners or self.coordinate_mapping != "ball_to_cube_volume_preserving"
                or self.interpolation != "linear" or not ops.cconv_scatter_supported(self.kernel, 1, 1)):
            return None
        info = lattice.lookup(out_positions)
        if info is None or not (info.voxel[0] == info.voxel[1] == info.voxel[2]) or max(info.dims) > SCATTER_MAX_LATTICE_CELLS:
            return None
        return info

    def _scatter_form(self, inp_features, inp_positions, out_positions, inp_importance, hash_table, radius):
        """(voxel, block_cells) if dmcf_cconv_scatter_forward applies to this call (_scatter_lattice) and is the faster forward:
        few output channels, many inputs, and inputs that are not a lattice of the outputs' family (then the stencil form
        applies)."""
        if os.environ.get("DMCF_SCATTER_CONV", "1") == "0" or inp_positions.shape[0] < SCATTER_MIN_INPUTS:
            return None
        if self.filters not in SCATTER_OUT_CHANNELS:
            return None
        info = self._scatter_lattice(inp_features, out_positions, inp_importance, hash_table)
        if info is None:
            return None
        m = ops.scatter_block_cells(self.filters, ops.scatter_reach(radius, info.voxel[0]))
        if m < 1 or out_positions.shape[0] * 4 > inp_positions.shape[0]:
            return None  # (a fine lattice: few pairs per flushed slot, the gather form is faster -- DESIGN.md section 4.2, splat S)
        return info.voxel[0], m

    def _scatter_train_form(self, inp_features, inp_positions, out_positions, inp_importance, hash_table):
        """Does dmcf_cconv_scatter_backward apply to this recording call: _scatter_form's conditions with every output channel
        count the library takes (4 or 8) and without those that only decide which FORWARD is faster (the input count, the
        lattice's fineness, the box fit, the channel list, DMCF_SCATTER_CONV)."""
        return self._scatter_lattice(inp_features, out_positions, inp_importance, hash_table) is not None

    def _lattice_form(self, inp_features, inp_positions, out_positions, inp_importance, hash_table, extent):
        """The LatticePair for this call if dmcf_lattice_conv_forward applies: both position tensors registered grid_pos
        lattices of one family (dmcf_amd/lattice.py), a named window, none of the options that form needs a pair list for."""
        from .. import lattice
        if (hash_table is not None or inp_importance is not None or self.symmetric or self.circular or self.normalize
                or not isinstance(self.window_function, WindowFunction) or self.radius_search_ignore_query_points
                or self.radius_search_metric != "L2" or not inp_features.is_cuda
                or self.in_channels not in (4, 8) or self.filters > 32):
            return None
        # (None too when the scene reaches so far from the origin that the nominal offsets d * voxel of this form and the
        # reference's differences of rounded positions part by more than the parity bar allows: lattice.MAX_X_OVER_EXTENT)
        lp = lattice.pair(inp_positions, out_positions, extent)
        if lp is not None:
            # a bounding box blown up by stray particles (a splash, a particle that left the scene): the dense zero-filled
            # volume would be mostly empty, or not fit the kernel's 32-bit addressing -- the neighbour-list form does not care
            cells = lp.volume_cells(ops, extent, inp_features.device)
            if (cells * self.in_channels > lattice.MAX_VOLUME_FLOATS
                    or cells > max(1 << 20, lattice.MAX_CELLS_PER_POINT * inp_positions.shape[0])):
                return None
        return lp

    call = forward

    @property
    def _avg_neighbors(self):
        """pairs / outputs of the last call (convolutions.py:385-388); synchronises when read."""
        pairs = self._pairs_last
        if hasattr(pairs, "total_ref"):  # (the list itself: its total is formed now, not in every step)
            pairs = pairs.total_ref
        pairs = int(pairs.item()) if isinstance(pairs, torch.Tensor) else pairs
        return pairs / max(self._n_out_last, 1)

    def compute_output_shape(self, inp_features_shape):
        return (None, self.filters)


class PointSampling(PlainAttributes, torch.nn.Module):
    """Mirror of the reference's ``PointSampling`` (utils/convolutions.py:888-1061): resamples features from one
    point set to another -- a ContinuousConv with a fixed 1x1x1 identity filter, optional window and
    normalisation by the summed window values.  Used by ``dens_norm`` to carry the density to the coarse
    point sets (models/pbf_model.py:177-181, 421-431)."""

    # ml3d.ops.continuous_conv with its defaults (:1038-1052) -- irrelevant for a one-cell filter, every neighbour puts all its
    # weight on that cell
    GEOMETRY = dict(align_corners=False, coordinate_mapping="ball_to_cube_radial", interpolation="linear")

    def __init__(self, window_function=None, normalize=True, name=None, **kwargs):
        super().__init__()
        self.normalize = normalize
        self.window_function = window_function
        self.fixed_radius_search = ops.FixedRadiusSearch(metric="L2", ignore_query_point=False,
                                                         return_distances=window_function is not None)
        self.radius_search = ops.RadiusSearch(metric="L2", ignore_query_point=False, return_distances=window_function is not None,
                                              normalize_distances=window_function is not None)
        self.kernel = None
        self.nns = None
        self.layer_name = name

    def build(self, in_channels, device=None):  # :925-929
        self.in_channels = in_channels
        self.kernel = torch.eye(in_channels, dtype=torch.float32, device=device).reshape(1, 1, 1, in_channels, in_channels)

    def forward(self, inp_features, inp_positions, out_positions, extents, inp_importance=None,
                fixed_radius_search_hash_table=None, user_neighbors_index=None, user_neighbors_row_splits=None,
                user_neighbors_importance=None):
        if self.kernel is None or self.kernel.shape[-1] != inp_features.shape[-1] or self.kernel.device != inp_features.device:
            self.build(inp_features.shape[-1], inp_features.device)
        users = (user_neighbors_index, user_neighbors_row_splits, user_neighbors_importance)
        n_pairs_ref = None
        if _rank1_extents(extents, out_positions):  # :1006-1010, the reference's defect and its reading as in ContinuousConv
            extent = extents
            lists = _extents_lists(self, inp_positions, out_positions, extents, *users)
        else:
            extent = float(np.float32(_scalar_extent(extents, "1006-1012")))
            lists = _callers_list(*users)
            if lists is None:
                radius = _search_radius(extent)
                if fixed_radius_search_hash_table is not None:
                    self.nns = self.fixed_radius_search(inp_positions, out_positions, radius,
                                                        hash_table=fixed_radius_search_hash_table)
                else:
                    self.nns = _CACHE.search(self.fixed_radius_search, inp_positions, out_positions, radius,
                                             distances=not isinstance(self.window_function, WindowFunction))
                n_pairs_ref = pairs_ref(self.nns)
                lists = _window_operands(self.window_function, self.nns, radius)
        neighbors_index, neighbors_row_splits, row_count, window, window_fac, neighbors_value = lists
        self._n_out_last = out_positions.shape[0]
        self._pairs_last = n_pairs_ref if n_pairs_ref is not None else (self.nns if user_neighbors_index is None else neighbors_index.shape[0])
        out = ops.cconv_forward(self.kernel, out_positions, extent, inp_positions, inp_features, neighbors_index,
                                neighbors_row_splits, neighbors_value=neighbors_value, window=window, window_fac=window_fac,
                                inp_importance=inp_importance, **self.GEOMETRY, normalize=self.normalize, n_pairs_ref=n_pairs_ref,
                                neighbors_row_count=row_count)
        self._conv_output = None if _CACHE.depth > 0 else out  # see ContinuousConv._keep_operands
        return out

    call = forward


class _SparseBase(PlainAttributes, torch.nn.Module):
    """What SparseConv and SparseConvTranspose share (the reference's :525-588 and :724-787): constructor keywords, the lazy
    weights, the max-norm search."""

    def __init__(self, filters, kernel_size, activation=None, use_bias=True, kernel_initializer="uniform", bias_initializer="zeros",
                 kernel_regularizer=None, bias_regularizer=None, normalize=False, offset=None, in_channels=None, name=None,
                 trainable=True, device=None, **kwargs):
        super().__init__()
        self.layer_name = name
        self.filters = filters
        self.kernel_size = [int(k) for k in kernel_size]
        if len(self.kernel_size) != 3:
            raise ValueError("kernel_size must be [kz, ky, kx]")
        if activation not in _ACTIVATIONS and not callable(activation):
            raise NotImplementedError(f"activation {activation!r}")
        self.activation = _ACTIVATIONS.get(activation, activation) if not callable(activation) else activation
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.normalize = normalize
        if offset is None:  # :553-559
            offset = torch.zeros(3) if self.kernel_size[0] % 2 else torch.full((3,), -0.5)
        self.offset = torch.as_tensor(offset, dtype=torch.float32).reshape(3).cpu()
        self.fixed_radius_search = ops.FixedRadiusSearch(metric="Linf", ignore_query_point=False, return_distances=False)
        self.in_channels = None
        self.kernel = None
        self.bias = None
        self._device = device
        self._avg_neighbors = None
        self._conv_values = None
        self._conv_output = None

    def build(self, in_channels, device=None):
        device = device or self._device or "cuda"
        self.in_channels = int(in_channels)
        kshape = (*self.kernel_size, self.in_channels, self.filters)
        self.kernel = torch.nn.Parameter(_init_tensor(self.kernel_initializer, kshape, device), requires_grad=False)
        if self.use_bias:
            self.bias = torch.nn.Parameter(_init_tensor(self.bias_initializer, (self.filters,), device), requires_grad=False)

    def _prepare(self, inp_features, voxel_size):
        if self.kernel is None:
            with torch.no_grad():
                self.build(inp_features.shape[-1], inp_features.device)
        if isinstance(voxel_size, torch.Tensor):
            if voxel_size.dim() != 0:
                raise ValueError("voxel_size must be a scalar")
            voxel_size = float(voxel_size)
        elif np.ndim(voxel_size) != 0:
            raise ValueError("voxel_size must be a scalar")
        voxel = np.float32(voxel_size)
        # :637 radius = kernel_size[-1] * voxel_size * 0.51, in float32
        radius = np.float32(np.float32(np.float32(self.kernel_size[-1]) * voxel) * np.float32(0.51))
        return float(voxel), float(radius)

    def _finish(self, out_features):
        self._conv_output = out_features
        if self.activation is not None:
            out_features = self.activation(out_features)
        return out_features


class SparseConv(_SparseBase):
    """Mirror of the reference's ``SparseConv`` (utils/convolutions.py:476-675): a convolution evaluated at the output positions
    only, for points on a regular grid -- each neighbour within ``kernel_size[-1] * voxel_size * 0.51`` in the max norm multiplies
    the one filter cell its relative position rounds to.  Same constructor keywords and ``call`` signature; ``kernel`` and
    ``bias`` are built at the first call with ``requires_grad=False`` (``requires_grad_(True)`` makes a call record).
    ``fixed_radius_search_hash_table``: an ``ops.build_spatial_hash_table`` result of ``inp_positions`` at that radius.

    Two side attributes differ from the reference's (both layers): ``_conv_output`` is the output with the bias already added --
    the kernel fuses it, where the reference keeps the operator's output before the bias (:666, :876) -- and ``_conv_values``
    holds the keywords of ``ops.sparse_conv`` / ``ops.sparse_conv_transpose`` (``voxel_size`` in place of ``extents``,
    ``align_corners``, ``coordinate_mapping`` and ``interpolation``, which are fixed on this path)."""

    def forward(self, inp_features, inp_positions, out_positions, voxel_size, inp_importance=None,
                fixed_radius_search_hash_table=None):
        voxel, radius = self._prepare(inp_features, voxel_size)
        offset = self.offset
        queries = out_positions - (offset * voxel).to(out_positions.device) if bool(offset.ne(0).any()) else out_positions
        self.nns = self.fixed_radius_search(inp_positions, queries=queries, radius=radius, hash_table_size_factor=1 / 64,
                                            hash_table=fixed_radius_search_hash_table)
        self._avg_neighbors = self.nns.neighbors_index.shape[0] / max(out_positions.shape[0], 1)
        self._conv_values = {
            "filters": self.kernel, "out_positions": out_positions, "voxel_size": voxel, "offset": offset,
            "inp_positions": inp_positions, "inp_features": inp_features, "inp_importance": inp_importance,
            "neighbors_index": self.nns.neighbors_index, "neighbors_row_splits": self.nns.neighbors_row_splits,
            "normalize": self.normalize,
        }
        return self._finish(ops.sparse_conv(**self._conv_values, bias=self.bias if self.use_bias else None))

    call = forward


class SparseConvTranspose(_SparseBase):
    """Mirror of the reference's ``SparseConvTranspose`` (utils/convolutions.py:678-885): the search runs from the INPUT points
    over the output points (``nns_inp``), the list is inverted, and every output point sums ``W[cell(out - inp)]^T f`` over the
    input points that found it; ``normalize`` divides an input's features by the number of outputs it reaches."""

    def forward(self, inp_features, inp_positions, out_positions, voxel_size, out_importance=None,
                fixed_radius_search_hash_table=None):
        voxel, radius = self._prepare(inp_features, voxel_size)
        offset = self.offset
        queries = inp_positions - (offset * voxel).to(inp_positions.device) if bool(offset.ne(0).any()) else inp_positions
        self.nns_inp = self.fixed_radius_search(out_positions, queries=queries, radius=radius, hash_table_size_factor=1 / 64,
                                                hash_table=fixed_radius_search_hash_table)
        inv = ops.invert_neighbors_list(out_positions.shape[0], self.nns_inp.neighbors_index, self.nns_inp.neighbors_row_splits)
        total = self.nns_inp.neighbors_index.shape[0]
        self._avg_neighbors = total / max(out_positions.shape[0], 1)
        self._conv_values = {
            "filters": self.kernel, "out_positions": out_positions, "voxel_size": voxel, "offset": offset,
            "inp_positions": inp_positions, "inp_features": inp_features, "out_importance": out_importance,
            "inp_neighbors_index": self.nns_inp.neighbors_index, "inp_neighbors_row_splits": self.nns_inp.neighbors_row_splits,
            "neighbors_index": inv.neighbors_index, "neighbors_row_splits": inv.neighbors_row_splits,
            "normalize": self.normalize,
        }
        return self._finish(ops.sparse_conv_transpose(**self._conv_values, bias=self.bias if self.use_bias else None))

    call = forward
