"""PointNet -- mirror of the reference's ``models/pointnet.py:12-195``: the particle baseline without convolutions.  Every
layer is a Dense followed by a sum over the fixed-radius neighbours (one dmcf_neighbor_dense_forward launch per layer).

Reference defect, reproduced: with ``use_bnds`` layer 0 gathers from ``dense_0(relu(fluid_feats))`` -- fluid rows only --
with neighbour indices over fluid AND boundary points (pointnet.py:137-145).  TensorFlow's GPU gather returns zeros for the
out-of-range rows and its gradient drops them (on the CPU it would raise), and the reference was trained on the GPU: so a
neighbour index >= the layer's input rows contributes nothing, neither features nor bias, forward or backward.  From layer 1
on every row exists and the layer outputs have n_fluid + n_box rows."""
import numpy as np
import torch

from .. import ops
from ..utils.tools.losses import compute_density, compute_pressure, compute_transformed_dx, get_dilated_pos, get_window_func
from .base_model import Dense
from .pbf_model import PBFNet


class PointNet(PBFNet):
    sharded_step_supported = False  # (dmcf_amd/parallel.py: its layers have no ghost exchange)

    def __init__(self, name="CConv", layer_channels=[32, 64, 64, 3], out_activation=None, **kwargs):
        self.layer_channels = layer_channels
        if out_activation == "tanh":
            self.out_activation = torch.tanh
        elif out_activation is None:
            self.out_activation = lambda x: x
        else:
            raise NotImplementedError()
        torch.nn.Module.__init__(self)
        super().__init__(name=name, channels=layer_channels[0], **kwargs)

    def setup(self):
        self.denses = []
        for i in range(len(self.layer_channels)):  # pointnet.py:30-36
            self.denses.append(Dense(units=self.layer_channels[i], name="dense{0}".format(i)))
        self._dense_modules = torch.nn.ModuleList(self.denses)

    def checkpoint_items(self):
        """The layers a TensorFlow checkpoint of this model holds: ``model/denses/{i}`` only -- PBFNet's input convolutions and
        Dense layers are never called here, so TensorFlow never builds them (utils/tf_checkpoint.py)."""
        return [([f"model/denses/{i}"], dense) for i, dense in enumerate(self.denses)]

    def preprocess(self, data, training=True, vel_corr=None, tape=None, **kwargs):
        """pointnet.py:38-125: the features [1, vel, acc (, feats, dens, pres)] of the fluid; no boundary crop, no input
        convolutions.  Returns [dilated_pos, fluid_feats, idx, dens]."""
        _pos, _vel, acc, feats, box, bfeats = data
        if vel_corr is not None:
            vel = vel_corr
            pos = _pos + vel * self.timestep
        else:
            pos, vel = self.integrate_pos_vel(_pos, _vel, acc)
        fluid_feats = [torch.ones_like(pos[:, :1])]
        if self.use_vel:
            fluid_feats.append(vel)
        if self.use_acc:
            if acc is None:
                raise ValueError("use_acc=True needs per-particle accelerations (pointnet.py:63-64)")
            fluid_feats.append(acc)
        if self.use_feats:
            fluid_feats.append(feats)
        box_feats = [torch.ones_like(box[:, :1])]
        if self.use_box_feats:
            box_feats.append(bfeats)
        all_pos = torch.cat([pos, box], dim=0)
        self.all_pos = all_pos
        dens = None
        if self.dens_feats or self.dens_norm or self.pres_feats:  # :74-88
            win = get_window_func(self.window_dens)
            dens = compute_density(all_pos, all_pos, self.dens_radius[0], win=win)
            n_fluid = pos.shape[0]
            if self.dens_feats:
                fluid_feats.append(dens[:n_fluid].unsqueeze(-1))
                box_feats.append(dens[n_fluid:].unsqueeze(-1))
            if self.pres_feats:
                pres = compute_pressure(all_pos, all_pos, dens, self.rest_dens, win=win, stiffness=self.stiffness)
                fluid_feats.append(pres[:n_fluid].unsqueeze(-1))
                box_feats.append(pres[n_fluid:].unsqueeze(-1))
        fluid_feats = torch.cat(fluid_feats, dim=-1)
        box_feats = torch.cat(box_feats, dim=-1)
        self.inp_feats = fluid_feats
        self.inp_bfeats = box_feats  # (built, not returned: as in the reference)
        dilated_pos, _, idx = get_dilated_pos(all_pos if self.use_bnds else pos, self.strides, voxel_size=self.voxel_size,
                                              centralize=self.centralize, pad=self.sample_pad, hyst=self.sample_hyst)  # :102-108
        if self.dens_norm:  # :110-120
            dens = [(dens if self.use_bnds else dens[:pos.shape[0]]).unsqueeze(-1)]
            for scale in range(1, len(self.dens_radius)):
                d = self.sampling(dens[-1], dilated_pos[scale - 1], dilated_pos[scale], self.dens_radius[scale], None)
                dens.append(torch.clamp(d, min=1e-2))
        else:
            dens = None
        self.dilated_pos = dilated_pos
        return [dilated_pos, fluid_feats, idx, dens]

    def forward(self, prev, data, training=True, **kwargs):
        """pointnet.py:127-147: one search (symmetric, self included), then per layer
        ans_i = sum_{neighbours} dense_i(relu(ans_{i-1})) (+ ans_{i-1} when the widths match), one launch each."""
        pos, feats = prev[:2]
        pos = pos[0]
        radius = float(np.float32(self.particle_radii[0]))
        nns = ops.FixedRadiusSearch()(pos, pos, radius)
        index, row_splits = nns.neighbors_index, nns.neighbors_row_splits
        self.neighbors_index, self.neighbors_row_splits = index, row_splits
        # the backward of every layer walks the inverse of this one list: inverted at most once per step
        shared = ops.SharedInverse(pos.shape[0], index, row_splits) if self.recording() else None
        ans = [feats]
        for i, dense in enumerate(self.denses):
            x = ans[-1]
            if dense.kernel is None:
                with torch.no_grad():
                    dense.build(x.shape[-1], x.device)
            residual = None
            if dense.units == x.shape[-1]:  # :144-145
                if x.shape[0] != pos.shape[0]:
                    # layer 0 with use_bnds: TensorFlow would fail adding [n_all, C] to [n_fluid, C]
                    raise ValueError("PointNet layer %d: a residual of %d rows for %d output rows (layer_channels[0] equals the "
                                     "input width)" % (i, x.shape[0], pos.shape[0]))
                residual = x
            ans.append(ops.neighbor_dense(x, dense.kernel, dense.bias, index, row_splits, relu=True, residual=residual,
                                          inverted=shared))
        return self.out_activation(ans[-1])

    def postprocess(self, prev, data, training=True, vel_corr=None, **kwargs):
        """pointnet.py:149-195."""
        pos, vel, acc = data[:3]
        pcnt = pos.shape[0]
        # every neighbour counts, boundary ones included (:158-160)
        self.num_fluid_neighbors = ops.neighbor_counts(self.neighbors_row_splits)[:pcnt]
        out = prev
        if self.equivar:  # :164-171
            scale = self.scale_dens(out)
            if scale.shape[0] != self.all_pos.shape[0]:
                raise NotImplementedError("equivar with use_bnds=False: the scale has %d rows for %d points (the reference's own "
                                          "gather is out of range there)" % (scale.shape[0], self.all_pos.shape[0]))
            out = compute_transformed_dx(self.all_pos, scale, None, radius=self.particle_radii[0])
        out_scale = ops.const_tensor(self.out_scale, torch.float32, pos.device)
        self.net_output = out
        self.pos_correction = out_scale * out[:pcnt]  # :178
        self.obs = out_scale * out[pcnt:]
        if vel_corr is not None:
            vel2 = vel_corr
            pos2 = pos + vel2 * self.timestep
        else:
            pos2, vel2 = self.integrate_pos_vel(pos, vel, acc)
        return list(self.compute_new_pos_vel(pos, vel, pos2, vel2, self.pos_correction))
