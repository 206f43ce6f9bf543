"""Window functions and multi-scale point sets -- mirror of the hot-path part of the reference's
``utils/tools/losses.py`` (same function names and arguments).

  get_window_func   losses.py:8-44     poly6 / cubic / linear / peak / cubic_grad on q = d^2/R^2
  grid_pos          losses.py:136-181  dilated voxel-corner lattice, de-duplicated (tf.unique order)
  get_dilated_pos   losses.py:249-284  one point set per stride (lattice with voxel_size, farthest point sampling without)

  compute_density   losses.py:285-306  windowed neighbour sum (fused into the search scan: ops.window_sum)
  compute_pressure  losses.py:367-377  Tait-style pressure from the density
  density_loss      losses.py:380-398  validation metric of pipelines/simulator.py:227-243
  emd_loss          losses.py:401-409  approximate-match EMD per batch item (ops.emd; differentiable in both sets with the
                                       match held constant, dmcf_emd_backward; with row splits a ragged batch in one
                                       call, dmcf_emd_ragged, no gradient)
  emd_loss_ragged   (no counterpart)   emd_loss of a ragged batch that can record: one dmcf_emd_ragged_with_levels call, one
                                       dmcf_emd_ragged_backward call

  get_loss          losses.py:47-110   the training losses mse / weighted_mse / vel / weighted_vel / momentum
  get_optimizer     models/pbf_model.py:508-517  Adam (eps 1e-6), piecewise-constant learning rate (torch.optim.Adam)
  KerasAdam         the same optimizer with Keras' update rule and state, on dmcf_adam_step: what the training loop uses

The density, Chamfer, EMD and histogram losses (losses.py:380-414, the last three on the reference's custom CUDA ops) are
not wired into get_loss: it returns a function that raises NotImplementedError for them.  The ops under them are
differentiable, so emd_loss and utils/tools/nn_distance.chamfer_loss can be added to an objective by hand.  So is the
density: compute_density, compute_pressure and density_loss are differentiable in the positions (ops.window_sum records
through dmcf_frs_window_sum_backward), which also carries the gradient of the models' dens_feats / pres_feats inputs.
"""
import numpy as np
import torch


class WindowFunction:
    """Callable returned by :func:`get_window_func`.

    Calling it on a tensor of normalised squared distances evaluates the formula with torch (generic
    use, e.g. user code).  ``ContinuousConv`` recognises the object and instead passes ``name`` /
    ``fac`` to the HIP kernel, which evaluates the same formula per neighbour inside the splat
    (dmcf_amd/csrc/cconv.hip: window_value) so no [P]-sized importance array is materialised.
    """

    def __init__(self, name, fac=1.0):
        self.name = name
        self.fac = float(fac)

    def __call__(self, q):
        fac = self.fac
        if self.name == "poly6":  # losses.py:11-12
            return fac * torch.clamp((1 - q) ** 3, 0, 1)
        if self.name == "cubic":  # losses.py:15-20
            s = torch.sqrt(q)
            inner = torch.where(s <= 0.5, 6 * (s ** 3 - q) + 1, 2 * (1 - s) ** 3)
            return fac * 4 / 3 * torch.where(q <= 1, inner, torch.zeros_like(s))
        if self.name == "linear":  # losses.py:23-25
            return fac * (1 - torch.sqrt(q))
        if self.name == "peak":  # losses.py:28-30
            return fac * (1 - 2 * torch.sqrt(q) + q)
        if self.name == "cubic_grad":  # losses.py:33-39
            s = torch.sqrt(q)
            inner = torch.where(s <= 0.5, 18 * q - 12 * s, -6 * (1 - s) ** 2)
            return fac * 4 / 3 * torch.where(q <= 1, inner, torch.zeros_like(s))
        raise NotImplementedError(self.name)

    def __repr__(self):
        return f"WindowFunction({self.name!r}, fac={self.fac})"


def get_window_func(typ, fac=1.0, **kwargs):
    """losses.py:8-44.  ``typ is None`` -> None (no window), unknown -> NotImplementedError."""
    if typ is None:
        return None
    if typ in ("poly6", "cubic", "linear", "peak", "cubic_grad"):
        return WindowFunction(typ, fac)
    raise NotImplementedError()


def _unique_first_occurrence(idx):
    """tf.unique(idx)[0]: unique values in order of first appearance (losses.py:171)."""
    uniq, inverse = torch.unique(idx, sorted=True, return_inverse=True)
    first = torch.full((uniq.shape[0],), idx.shape[0], dtype=torch.int64, device=idx.device)
    first.scatter_reduce_(0, inverse, torch.arange(idx.shape[0], device=idx.device), reduce="amin")
    return uniq[torch.argsort(first)]


def _grid_pos_items(pos, voxel_size, centralize, pad, hyst, center, row_splits):
    """grid_pos of a batch of point sets: item b = pos[rs[b]:rs[b+1]] -> (points, ops.RowSplits).  On the device one
    batched call (csrc/grid.hip, dmcf_grid_pos_*_batched); on host tensors the loop over the items of the host formulation."""
    from ... import ops
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("pos must be [n, 3]")
    if pos.is_cuda:
        vs_host = np.asarray(voxel_size.detach().cpu() if isinstance(voxel_size, torch.Tensor) else voxel_size,
                             dtype=np.float32).reshape(3)
        return ops.grid_pos(pos, vs_host, centralize=centralize, pad=pad, hyst=hyst, center=center, row_splits=row_splits)
    host, _ = ops._host_row_splits(row_splits, "row_splits")
    ops._check_row_splits(host, pos.shape[0], "row_splits")
    batch = len(host) - 1
    if center is not None and tuple(center.shape) != (batch, 3):
        raise ValueError(f"center must be [batch, 3] = [{batch}, 3] with row_splits, got {tuple(center.shape)}")
    parts, out_host = [], [0]
    for b in range(batch):
        item = pos[host[b]:host[b + 1]]
        if item.shape[0]:  # (an empty item contributes no rows)
            parts.append(grid_pos(item, voxel_size, centralize=centralize, pad=pad, hyst=hyst,
                                  center=None if center is None else center[b]))
        out_host.append(out_host[-1] + (parts[-1].shape[0] if item.shape[0] else 0))
    out = torch.cat(parts, dim=0) if parts else pos.new_zeros((0, 3))
    return out, ops.RowSplits(tuple(out_host), torch.tensor(out_host, dtype=torch.int64, device=pos.device), False)


def grid_pos(pos, voxel_size, centralize=False, pad=0, hyst=0.1, center=None, return_box=False, row_splits=None):
    """losses.py:136-181: lattice corners of the voxels (edge ``voxel_size``) that contain a particle,
    with +-``hyst`` hysteresis; axes with voxel_size < 1e-5 collapse (2-D / 1-D scenes).
    ``center`` (extension used by the sharded path): the lattice origin to use instead of this call's own
    mean when ``centralize`` -- every rank passes the global mean so all ranks build the same lattice.
    ``return_box``: -> (points, (minp, dims) | None), the integer box of cells (x, y, z) that holds every returned point;
    None when it is not known on the host (empty result, or the sort-based fallback ran).
    ``row_splits``: ``pos`` is a batch of point sets, item b = pos[rs[b]:rs[b+1]] -> (points, ops.RowSplits): the items'
    lattices one after the other, each exactly what this call returns for the item alone; ``center`` is then [batch, 3]."""
    if row_splits is not None:
        if return_box:
            raise NotImplementedError("grid_pos: return_box with row_splits (a batch has one box per item)")
        return _grid_pos_items(pos, voxel_size, centralize, pad, hyst, center, row_splits)
    # voxel_size is kept on the host (list / numpy float32) so that the axis collapse test does not
    # force a device round trip; values are float32 like the reference's tf.constant
    vs_host = np.asarray(voxel_size.detach().cpu() if isinstance(voxel_size, torch.Tensor) else voxel_size,
                         dtype=np.float32).reshape(3)
    if pos.is_cuda:  # product path: the HIP kernels (csrc/grid.hip); below is the host-side form of the same
        from ... import ops
        try:
            out, box = ops.grid_pos(pos, vs_host, centralize=centralize, pad=pad, hyst=hyst, center=center, return_box=True)
            return (out, box) if return_box else out
        except ops.GridTooSparse:
            pass  # bounding box too large for a dense cell table: sort-based form, still on the device
    voxel_size = torch.from_numpy(vs_host.copy()).to(pos.device)
    if centralize:
        if center is None:
            center = pos.mean(dim=0)  # :138
        pos = pos - center
    active = voxel_size >= 1e-5
    vs = torch.clamp(voxel_size, min=1e-5)
    h = torch.where(active, torch.full_like(vs, hyst), torch.zeros_like(vs))
    scaled = pos / vs
    dpos = torch.cat([torch.floor(scaled - h).to(torch.int32), torch.floor(scaled + h).to(torch.int32)], dim=0)  # :142-150
    active_host = (vs_host >= 1e-5).tolist()
    ranges_host = [list(range(-pad, 2 + pad)) if a else [0] for a in active_host]  # :151-161
    ranges = [torch.tensor(r, device=pos.device) for r in ranges_host]
    offset = torch.stack(torch.meshgrid(*ranges, indexing="ij"), dim=-1).reshape(1, -1, 3).to(torch.int32)
    dpos = (dpos.unsqueeze(1) + offset).reshape(-1, 3)
    # :167-170 -- floor is monotone, so the extrema of the 16N candidate cells follow from the extrema of the N
    # scaled positions (a [16N,3] column reduction is ~8 ms per call on 18M rows; this one is ~0.5 ms)
    smin, smax = scaled.min(dim=0).values, scaled.max(dim=0).values
    off_lo = torch.tensor([r[0] for r in ranges_host], dtype=torch.int32, device=pos.device)
    off_hi = torch.tensor([r[-1] for r in ranges_host], dtype=torch.int32, device=pos.device)
    minp = torch.floor(smin - h).to(torch.int32) + off_lo
    maxp = torch.floor(smax + h).to(torch.int32) + off_hi - minp + 1
    maxp64 = maxp.to(torch.int64)
    mult = torch.stack([torch.ones_like(maxp64[0]), maxp64[0], maxp64[0] * maxp64[1]])
    idx = ((dpos - minp).to(torch.int64) * mult).sum(dim=-1)
    idx = _unique_first_occurrence(idx)  # :171
    gpos = torch.stack([idx % maxp64[0], idx // maxp64[0] % maxp64[1], idx // (maxp64[0] * maxp64[1])], dim=-1) \
        + minp.to(torch.int64)  # :172-174
    if centralize:
        out = gpos.to(torch.float32) * voxel_size + center  # :177
    else:
        out = gpos.to(torch.float32) * voxel_size + voxel_size / 2  # :179
    return (out, None) if return_box else out


def _get_dilated_pos_items(pos, strides, voxel_size, centralize, pad, hyst, row_splits):
    """get_dilated_pos of a batch of point sets -> (dilated_pos, pcnt, idx, level_row_splits): every level holds the items'
    point sets one after the other, level_row_splits[k] (ops.RowSplits) says where."""
    from ... import ops
    host, dev = ops._host_row_splits(row_splits, "row_splits")
    ops._check_row_splits(host, pos.shape[0], "row_splits")
    coarse = [s for s in strides if s != 1]
    if coarse and voxel_size is None:
        raise NotImplementedError("get_dilated_pos: farthest-point-sampled levels (voxel_size=None) with row_splits")
    rs_dev = dev if dev is not None and dev.device == pos.device else torch.tensor(host, dtype=torch.int64, device=pos.device)
    own = ops.RowSplits(host, rs_dev, False)
    lattices = {}
    if coarse:
        vs = voxel_size.detach().cpu().numpy() if isinstance(voxel_size, torch.Tensor) else voxel_size
        sizes = [np.asarray(vs, dtype=np.float32) * np.float32(s) for s in coarse]  # :266
        if pos.is_cuda:  # all levels in one go: two host round trips for all of them
            res = ops.grid_pos_many(pos, sizes, centralize=centralize, pad=pad, hyst=hyst, row_splits=own)
        else:
            res = [grid_pos(pos, v, centralize=centralize, pad=pad, hyst=hyst, row_splits=host) for v in sizes]
        lattices = dict(zip(coarse, res))
    dilated_pos, pcnt, idx, level_rs = [], [], [], []
    for stride in strides:
        if stride == 1:
            dilated_pos.append(pos)
            idx.append(None)
            level_rs.append(own)
        else:
            dilated_pos.append(lattices[stride][0])
            level_rs.append(lattices[stride][1])
        pcnt.append(dilated_pos[-1].shape[0])
    return dilated_pos, pcnt, idx, level_rs


def get_dilated_pos(pos, strides, voxel_size=None, centralize=False, pad=0, hyst=0.1, row_splits=None):
    """losses.py:249-284 -> (dilated_pos, pcnt, idx).  With ``voxel_size`` every coarse level is a lattice computed from
    the full-resolution set (:266-272; no entry is appended to ``idx`` on that branch, as in the reference); without it
    level k is ``n // stride`` farthest-point samples of level k-1 (:274-282) and ``idx[k]`` the [1, m] sample indices
    HRNet's cross-scale Dense branch uses.
    ``row_splits``: ``pos`` is a batch of point sets -> (dilated_pos, pcnt, idx, level_row_splits), see
    :func:`_get_dilated_pos_items`; farthest-point-sampled levels raise NotImplementedError."""
    if row_splits is not None:
        return _get_dilated_pos_items(pos, strides, voxel_size, centralize, pad, hyst, row_splits)
    from ... import ops
    pcnt, dilated_pos, idx = [], [], []
    lattices = {}
    if voxel_size is not None:
        vs = voxel_size.detach().cpu().numpy() if isinstance(voxel_size, torch.Tensor) else voxel_size
        coarse = [s for s in strides if s != 1]
        if pos.is_cuda and len(coarse) > 1:
            # every coarse level is built from the SAME positions: their kernels are enqueued together and the host waits twice
            # for all of them, not twice per level (a step of the 2-D models is paced by its host round trips)
            try:
                res = ops.grid_pos_many(pos, [np.asarray(vs, dtype=np.float32) * np.float32(s) for s in coarse],
                                        centralize=centralize, pad=pad, hyst=hyst)
                lattices = {s: r[0] for s, r in zip(coarse, res)}
            except ops.GridTooSparse:
                lattices = {}  # (a level's box is too sparse for the dense cell table: one at a time, each in the form it needs)
    for stride in strides:
        if stride == 1:
            pcnt.append(pos.shape[0])
            dilated_pos.append(pos)
            idx.append(None)
        elif voxel_size is not None:
            if stride in lattices:
                dilated_pos.append(lattices[stride])
            else:
                v_scale = np.asarray(vs, dtype=np.float32) * np.float32(stride)  # :266
                dilated_pos.append(grid_pos(pos, v_scale, centralize=centralize, pad=pad, hyst=hyst))
            pcnt.append(dilated_pos[-1].shape[0])
        else:
            sample_cnt = max(pos.shape[0] // stride, 1)  # :275
            pcnt.append(sample_cnt)
            idx.append(ops.farthest_point_sample(sample_cnt, dilated_pos[-1].unsqueeze(0)))
            dilated_pos.append(ops.gather_point(dilated_pos[-1].unsqueeze(0), idx[-1])[0])
    return dilated_pos, pcnt, idx


def _density_row_splits(out_pos, in_pos, out_row_splits, in_row_splits, names):
    """The host-side checks of the batched density functions, all before a device is touched: both splits or neither
    (``in_pos is None`` takes the out splits), well-formed, equal batch.  -> (out splits, in splits) as ops.RowSplits whose
    device copies live on ``out_pos``'s device when that is a GPU (made once here, shared by every call that follows)."""
    from ... import ops
    if in_pos is None and in_row_splits is None:
        in_row_splits = out_row_splits
    if out_row_splits is None or in_row_splits is None:
        raise NotImplementedError(f"the batched density needs both {names[0]} and {names[1]}")
    if ops.SEARCH_SETS[ops.search_set()] != 0:
        raise NotImplementedError(f"DMCF_FRS_SET={ops.search_set()} has no batched form: the open3d walk emulations know nothing of items")
    (o_host, o_dev), (i_host, i_dev) = ops._batched_row_splits(out_pos if in_pos is None else in_pos, out_pos, in_row_splits,
                                                               out_row_splits)[::-1]
    if out_pos.is_cuda:
        same = in_row_splits is out_row_splits
        o_dev = ops._row_splits_on(o_host, o_dev, out_pos.device)
        i_dev = o_dev if same else ops._row_splits_on(i_host, i_dev, out_pos.device)
    return ops.RowSplits(o_host, o_dev), ops.RowSplits(i_host, i_dev)


def _item_of_rows(row_splits, device):
    """[n] int64: the batch item of every row."""
    counts = torch.diff(row_splits.dev if row_splits.dev is not None else torch.tensor(row_splits.host, device=device))
    return torch.repeat_interleave(torch.arange(len(row_splits.host) - 1, device=device), counts, output_size=row_splits.host[-1])


def _compute_density_batched(out_pos, in_pos, radius, win, out_rs, in_rs, want_max=False):
    """compute_density with row splits (validated: ops.RowSplits) -> dens, or (dens, item_max [batch]) with ``want_max``."""
    from ... import ops
    if in_pos is None:
        in_pos = out_pos
    radius = float(radius)
    batch = len(out_rs.host) - 1
    if win is None or isinstance(win, WindowFunction):
        name = "explicit" if win is None else win.name
        fac = 1.0 / (radius * radius) if win is None else win.fac
        fused_max = want_max and name != "cubic_grad" and fac > 0  # (the kernel's maximum orders non-negative sums; scaling by fac > 0 keeps the order)
        res = ops.window_sum(in_pos, out_pos, radius, name, points_row_splits=in_rs, queries_row_splits=out_rs,
                             return_item_max=fused_max)
        d, mx = res if fused_max else (res, None)
        if win is None:
            d = d / (radius * radius)
            mx = None if mx is None else mx / (radius * radius)
        elif fac != 1.0:
            d = d * fac
            mx = None if mx is None else mx * fac
    else:
        nns = ops.fixed_radius_search(in_pos, out_pos, radius, return_distances=True, points_row_splits=in_rs,
                                      queries_row_splits=out_rs)
        d = ops.reduce_subarrays_sum(win(nns.neighbors_distance / (radius * radius)), nns.neighbors_row_splits)
        mx = None
    if not want_max:
        return d
    if mx is None:
        mx = torch.zeros(batch, dtype=d.dtype, device=d.device).scatter_reduce(0, _item_of_rows(out_rs, d.device), d.detach(), "amax",
                                                                               include_self=False)
    return d, mx


def compute_density(out_pos, in_pos=None, radius=0.005, win=None, out_row_splits=None, in_row_splits=None):
    """losses.py:285-306: ``dens[i] = sum_j win(|in_pos[j] - out_pos[i]|^2 / radius^2)`` over the points within
    ``radius`` (the query point itself included).  ``win``: an object from :func:`get_window_func` (evaluated inside
    the search kernel, no pair list), None (the reference warns and uses the identity: sum of q), or any callable
    on a tensor of q values (evaluated with torch on the pair list).  Differentiable in both position sets for a window
    object and for None (ops.window_sum); a callable is evaluated on the search's distances, which carry no gradient.

    ``out_row_splits`` / ``in_row_splits`` (both or neither; ``in_pos=None`` takes the out splits): the densities of a BATCH of
    point sets in one call, a point summing over the ``in_pos`` of its own item only (the batched ops.window_sum /
    ops.fixed_radius_search)."""
    from ... import ops
    if out_row_splits is not None or in_row_splits is not None:
        out_rs, in_rs = _density_row_splits(out_pos, in_pos, out_row_splits, in_row_splits, ("out_row_splits", "in_row_splits"))
        return _compute_density_batched(out_pos, in_pos, radius, win, out_rs, in_rs)
    if in_pos is None:
        in_pos = out_pos
    radius = float(radius)
    if win is None:
        return ops.window_sum(in_pos, out_pos, radius, "explicit") / (radius * radius)
    if isinstance(win, WindowFunction):
        d = ops.window_sum(in_pos, out_pos, radius, win.name)
        return d if win.fac == 1.0 else d * win.fac
    nns = ops.fixed_radius_search(in_pos, out_pos, radius, return_distances=True)
    return ops.reduce_subarrays_sum(win(nns.neighbors_distance / (radius * radius)), nns.neighbors_row_splits)


def compute_transformed_dx(pos, scale=None, rot=None, radius=0.005):
    """losses.py:337-364: per point the MEAN over its neighbours within ``radius`` (itself included) of ``(x_j - x_i) *
    scale_j``.  The reference's caller passes ``rot=None`` (models/pbf_model.py:458-460 has the quaternion branch commented
    out); a rotation raises here.  The pair list comes from the fixed-radius search, the ragged sums from
    dmcf_reduce_subarrays_sum; a point without neighbours gives 0 / 0 = NaN as tf.reduce_mean over an empty row does."""
    from ... import ops
    if rot is not None:
        raise NotImplementedError("compute_transformed_dx with a rotation (quat_mean / quat_rot): the reference never passes one")
    nns = ops.fixed_radius_search(pos, pos, float(radius), return_distances=False)
    idx, rs = nns.neighbors_index.long(), nns.neighbors_row_splits
    counts = torch.diff(rs)
    row = torch.repeat_interleave(torch.arange(pos.shape[0], device=pos.device), counts, output_size=idx.shape[0])
    dx = pos[idx] - pos[row]
    if scale is not None:
        dx = dx * scale[idx]
    sums = torch.stack([ops.reduce_subarrays_sum(dx[:, k].contiguous(), rs) for k in range(dx.shape[1])], dim=1)
    return sums / counts.to(sums.dtype).unsqueeze(1)


def compute_pressure(out_pts, inp_pts=None, dens=None, rest_dens=3.5, stiffness=20.0, win=None):
    """losses.py:367-377 (note: the reference ignores a radius here too: compute_density's default applies).  Differentiable in
    the positions through compute_density."""
    if inp_pts is None:
        inp_pts = out_pts
    if dens is None:
        dens = compute_density(out_pts, inp_pts, win=win)
    return torch.relu(stiffness * ((dens / rest_dens) ** 7 - 1))


def density_loss(gt, pred, gt_in=None, pred_in=None, radius=0.005, eps=0.01, win=None, use_max=False, row_splits=None,
                 in_row_splits=None, **kwargs):
    """losses.py:380-398.  Differentiable in ``pred`` and ``pred_in`` (compute_density); not wired into get_loss.

    ``row_splits`` (shared by ``gt`` and ``pred``) / ``in_row_splits`` (shared by ``gt_in`` and ``pred_in``; without the in sets
    the row splits serve): a BATCH of items in one call -> [batch], entry b what the un-batched call returns on item b's slices.
    ``use_max=True`` takes both maxima per item from the window-sum kernel (which carry no gradient: the batched form is the
    warm-up's check, not a training loss); otherwise the mean of the relu term per item, differentiable as before.  An
    item without rows is a ValueError (the un-batched call cannot take the maximum of nothing either)."""
    if row_splits is not None or in_row_splits is not None:
        if (gt_in is None) != (pred_in is None):
            raise NotImplementedError("the batched density_loss needs gt_in and pred_in both or neither: they share in_row_splits")
        if gt.shape[0] != pred.shape[0] or (gt_in is not None and gt_in.shape[0] != pred_in.shape[0]):
            raise ValueError("gt and pred (and gt_in and pred_in) must have equal numbers of rows: they share their row splits")
        out_rs, in_rs = _density_row_splits(gt, gt_in, row_splits, in_row_splits, ("row_splits", "in_row_splits"))
        batch = len(out_rs.host) - 1
        empty = [b for b in range(batch) if out_rs.host[b + 1] == out_rs.host[b]]
        if empty:
            raise ValueError(f"density_loss: items {empty} have no rows (the maximum of nothing)")
        pred_dens, pred_max = _compute_density_batched(pred, pred_in, radius, win, out_rs, in_rs, want_max=True)
        _, rest_dens = _compute_density_batched(gt, gt_in, radius, win, out_rs, in_rs, want_max=True)
        if use_max:
            return torch.abs(pred_max - rest_dens) / rest_dens
        item = _item_of_rows(out_rs, pred_dens.device)
        term = torch.relu(pred_dens - rest_dens[item] - eps)
        counts = torch.diff(out_rs.dev).to(term.dtype)
        return torch.zeros(batch, dtype=term.dtype, device=term.device).index_add(0, item, term) / counts
    pred_dens = compute_density(pred, pred_in, radius, win=win)
    gt_dens = compute_density(gt, gt_in, radius, win=win)
    rest_dens = gt_dens.max()
    if use_max:
        return torch.abs(pred_dens.max() - rest_dens) / rest_dens
    return torch.relu(pred_dens - rest_dens - eps).mean()


def emd_loss(y_true, y_pred, n=None, m=None, true_row_splits=None, pred_row_splits=None):
    """losses.py:401-409: ``match_cost(approx_match(y_true, y_pred, n, m)) / max(n, m)`` per batch item, [b].  ``y_true``
    [b, n, 3], ``y_pred`` [b, m, 3] (2-D: z = 0); ``n`` / ``m`` per-batch point counts (None: all points).  Runs the fused
    kernel (ops.emd), which never forms the [b, m, n] match.  Differentiable in ``y_true`` and ``y_pred`` with the match held
    constant (approx_match has no gradient), through dmcf_emd_backward, which does not form the match either.

    ``true_row_splits`` / ``pred_row_splits`` (both or neither, and then no ``n`` / ``m``): a RAGGED batch in one call
    (ops.emd with row splits), ``y_true`` [n_total, 3] and ``y_pred`` [m_total, 3]; -> ``cost / max(n_b, m_b)`` per item,
    [batch], with the bits of the call on every item alone; an item with both sets empty gives 0.  No gradient here:
    :func:`emd_loss_ragged` with ``record=True`` is the form that trains."""
    from ... import ops
    if true_row_splits is not None or pred_row_splits is not None:
        cost = ops.emd(y_true, y_pred, n, m, row_splits1=true_row_splits, row_splits2=pred_row_splits)
        s1 = np.asarray(ops._host_row_splits(true_row_splits, "true_row_splits")[0])
        s2 = np.asarray(ops._host_row_splits(pred_row_splits, "pred_row_splits")[0])
        denom = np.maximum(np.maximum(np.diff(s1), np.diff(s2)), 1)  # (both sets empty: cost 0 over 1)
        return cost / torch.from_numpy(denom.astype(np.float32)).to(cost.device)
    b = y_true.shape[0]
    nn_ = ops._host_counts(n, b, y_true.shape[1], "n")
    mm = ops._host_counts(m, b, y_pred.shape[1], "m")
    cost = ops.emd(y_true, y_pred, nn_, mm)
    nv = np.full(b, y_true.shape[1]) if nn_ is None else nn_
    mv = np.full(b, y_pred.shape[1]) if mm is None else mm
    denom = torch.from_numpy(np.maximum(nv, mv).astype(np.float32)).to(cost.device)
    return cost / denom


def emd_loss_ragged(y_true, y_pred, true_row_splits, pred_row_splits, record=False):
    """:func:`emd_loss` of a RAGGED batch, ``y_true`` [n_total, 3|2] and ``y_pred`` [m_total, 3|2] with their row splits ->
    ``cost / max(n_b, m_b, 1)`` per item, [batch], with the bits of the call on every item alone.  ``record=True``:
    differentiable in both sets with the match held constant (ops.emd_ragged_recording: one recording forward, one
    dmcf_emd_ragged_backward call for the whole batch; the divisor is a constant), every item's gradient rows with the bits of
    emd_loss on the item alone.  ``record=False`` is emd_loss with row splits: inputs that require grad raise
    NotImplementedError."""
    from ... import ops
    cost = (ops.emd_ragged_recording if record else ops.emd_ragged)(y_true, y_pred, true_row_splits, pred_row_splits)
    s1 = np.asarray(ops._host_row_splits(true_row_splits, "true_row_splits")[0])
    s2 = np.asarray(ops._host_row_splits(pred_row_splits, "pred_row_splits")[0])
    denom = np.maximum(np.maximum(np.diff(s1), np.diff(s2)), 1)  # (both sets empty: cost 0 over 1)
    return cost / torch.from_numpy(denom.astype(np.float32)).to(cost.device)


def _pre_factor(kwargs, kw, like):
    # tf.exp(-pre_scale * float(pre_steps)) (losses.py:51-52)
    steps = kw.get("pre_steps")
    steps = 0.0 if steps is None else steps
    return torch.exp(-float(kwargs.get("pre_scale", 0.0)) * torch.as_tensor(steps, dtype=torch.float32, device=like.device))


def get_loss(typ, fac=1.0, **kwargs):
    """losses.py:47-110: the loss function of one entry of a config's ``loss`` section, called as ``f(target, pred, **kw)``
    with the keywords of PBFNet.loss (num_fluid_neighbors, input, target_prev, pre_steps, pos_correction)."""
    gamma = kwargs.get("gamma", 0.5)
    if typ == "mse":
        def f(target, pred, **kw):
            diff = (torch.sum((target - pred) ** 2, dim=-1) + 1e-9) ** gamma
            return fac * torch.mean(_pre_factor(kwargs, kw, pred) * diff)
        return f
    if typ == "weighted_mse":
        def f(target, pred, **kw):
            importance = torch.exp(-kwargs.get("neighbor_scale", 1.0) * torch.as_tensor(kw.get("num_fluid_neighbors"),
                                                                                     dtype=torch.float32, device=pred.device))
            diff = (torch.sum((target - pred) ** 2, dim=-1) + 1e-9) ** gamma
            return fac * torch.mean(_pre_factor(kwargs, kw, pred) * importance * diff)
        return f
    if typ == "vel":
        def f(target, pred, **kw):
            inp, prev = kw.get("input")[0], kw.get("target_prev")
            diff = (torch.sum(((target - prev) - (pred - inp)) ** 2, dim=-1) + 1e-9) ** gamma
            return fac * torch.mean(diff)
        return f
    if typ == "weighted_vel":
        def f(target, pred, **kw):
            inp, prev = kw.get("input")[0], kw.get("target_prev")
            importance = torch.exp(-kwargs.get("neighbor_scale", 1.0) * torch.as_tensor(kw.get("num_fluid_neighbors"),
                                                                                     dtype=torch.float32, device=pred.device))
            diff = (torch.sum(((target - prev) - (pred - inp)) ** 2, dim=-1) + 1e-9) ** gamma
            return fac * torch.mean(importance * diff)
        return f
    if typ == "momentum":
        def f(target, pred, **kw):
            return fac * torch.mean(kw.get("pos_correction"))
        return f
    if typ in ("dense", "chamfer", "emd", "hist"):
        def f(*args, **kw):
            raise NotImplementedError(f"the {typ!r} training loss is not implemented")
        return f
    raise NotImplementedError(typ)


class PiecewiseConstant:
    """tf.keras.optimizers.schedules.PiecewiseConstantDecay(boundaries, values): values[0] for step <= boundaries[0],
    values[k] for boundaries[k-1] < step <= boundaries[k], values[-1] after the last boundary."""

    def __init__(self, boundaries, values):
        if len(values) != len(boundaries) + 1:
            raise ValueError("lr_values must have one entry more than lr_boundaries")
        self.boundaries = [int(b) for b in boundaries]
        self.values = [float(v) for v in values]

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]


def get_optimizer(params, cfg):
    """models/pbf_model.py:508-517: Adam with epsilon 1e-6 and the piecewise-constant learning rate of ``cfg['lr_boundaries']``
    / ``cfg['lr_values']``, as (optimizer, scheduler): call ``scheduler.step()`` after every ``optimizer.step()`` -- the
    learning rate of optimiser step k (counted from 0, as Keras' iterations) is PiecewiseConstant(...)(k).  This is torch's
    update rule (epsilon added to the bias-corrected sqrt(v)); the training loop (Simulator.run_train) uses :class:`KerasAdam`,
    the reference's rule and checkpoint state."""
    sched = PiecewiseConstant(cfg["lr_boundaries"], cfg["lr_values"])
    opt = torch.optim.Adam(params, lr=sched.values[0], eps=1e-6)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: sched(step) / sched.values[0])
    return opt, lam


class KerasAdam:
    """tf.keras.optimizers.Adam(learning_rate=PiecewiseConstantDecay(lr_boundaries, lr_values), epsilon=1e-6) of
    models/pbf_model.py:511-517, on the HIP kernel dmcf_adam_step (ops.adam_step).  For optimizer iteration t (``iterations``
    before the step, counted from 0): lr = the schedule at t (divided by ``1 + decay t`` when ``decay`` > 0, Keras'
    _decayed_lr), beta_*^(t + 1) in float32, and TensorFlow's ApplyAdam:
        alpha = lr sqrt(1 - beta_2^(t+1)) / (1 - beta_1^(t+1));  m += (1 - beta_1)(g - m);  v += (1 - beta_2)(g^2 - v)
        param -= alpha m / (epsilon + sqrt(v))
    -- epsilon is added to sqrt(v), not to the bias-corrected one as torch.optim.Adam does.  ``clip_norm`` > 0: each gradient
    is clipped first as tf.clip_by_norm does (the pipeline's ``grad_clip_norm``).

    State, named like a checkpoint's ``optimizer/*`` and ``.OPTIMIZER_SLOT/optimizer/{m,v}`` entries: ``iterations``,
    ``beta_1``, ``beta_2``, ``decay``, and the slots ``m`` / ``v`` (one per parameter, None until the parameter first has a
    gradient: as in Keras, a parameter whose gradient is None is neither updated nor given slots)."""

    def __init__(self, params, lr_boundaries=(), lr_values=(1e-3,), beta_1=0.9, beta_2=0.999, epsilon=1e-6, decay=0.0,
                 clip_norm=None):
        self.params = list(params)
        self.schedule = PiecewiseConstant(lr_boundaries, lr_values)
        self.beta_1, self.beta_2, self.epsilon, self.decay = float(beta_1), float(beta_2), float(epsilon), float(decay)
        self.clip_norm = clip_norm if clip_norm is not None and clip_norm > 0 else None
        self.iterations = 0
        self.m = [None] * len(self.params)
        self.v = [None] * len(self.params)

    @classmethod
    def from_config(cls, params, cfg, clip_norm=None):
        """The pipeline's ``optimizer:`` section (lr_boundaries, lr_values) -> the reference's optimizer."""
        return cls(params, cfg["lr_boundaries"], cfg["lr_values"], epsilon=1e-6, clip_norm=clip_norm)

    def lr(self, iterations=None):
        """Learning rate of optimizer iteration ``iterations`` (default: the next step's), float32 like Keras'."""
        t = self.iterations if iterations is None else int(iterations)
        lr = np.float32(self.schedule(t))
        if self.decay > 0:
            lr = np.float32(lr / (np.float32(1.0) + np.float32(self.decay) * np.float32(t)))
        return lr

    def coefficients(self, iterations=None):
        """(lr, beta_1^(t+1), beta_2^(t+1)) in float32 for iteration t (default: the next step's)."""
        t = self.iterations if iterations is None else int(iterations)
        step = np.float32(t + 1)
        return self.lr(t), np.power(np.float32(self.beta_1), step), np.power(np.float32(self.beta_2), step)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        """One update of every parameter that has a gradient; ``iterations`` += 1 (also when none has one, as Keras)."""
        from ... import ops
        live = [i for i, p in enumerate(self.params) if p.grad is not None]
        for i in live:
            if self.m[i] is None:
                self.m[i] = torch.zeros_like(self.params[i], memory_format=torch.contiguous_format)
                self.v[i] = torch.zeros_like(self.params[i], memory_format=torch.contiguous_format)
        lr, b1p, b2p = self.coefficients()
        if live:
            with torch.no_grad():
                ops.adam_step([self.params[i] for i in live], [self.params[i].grad.contiguous() for i in live],
                              [self.m[i] for i in live], [self.v[i] for i in live], lr, self.beta_1, self.beta_2,
                              self.epsilon, b1p, b2p, self.clip_norm)
            # the kernel wrote through raw pointers: advance the parameters' version counters as an in-place torch op would
            # (ops.cconv_forward's packed-filter cache is keyed on them)
            for i in live:
                torch.autograd.graph.increment_version(self.params[i])
        self.iterations += 1

    def slots_by_param(self):
        """{id(parameter): {'m': tensor, 'v': tensor}} for the parameters that have slots."""
        return {id(p): {"m": m, "v": v} for p, m, v in zip(self.params, self.m, self.v) if m is not None}

    def set_slots(self, param, m, v):
        """Restore the slots of ``param`` (arrays or tensors of its shape)."""
        i = next(k for k, p in enumerate(self.params) if p is param)
        as_t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(param.device).reshape(param.shape).contiguous()  # noqa: E731
        self.m[i], self.v[i] = as_t(m), as_t(v)
