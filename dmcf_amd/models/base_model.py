"""BaseModel -- mirror of the reference's ``models/base_model.py:10-107``: the five-stage ``call``."""
import torch

from ..utils.convolutions import PlainAttributes

from .. import ops
from ..utils.config import Config


class Dense(PlainAttributes, torch.nn.Module):
    """tf.keras.layers.Dense(units, activation=None): lazily built ``kernel`` [in, units] (glorot
    uniform) and ``bias`` [units] (zeros); dmcf_dense_forward for the shapes it takes (a row per thread), else torch's GEMM."""

    def __init__(self, units, name=None, activation=None, use_bias=True):
        super().__init__()
        assert activation is None
        self.units = units
        self.layer_name = name
        self.use_bias = use_bias
        self.kernel = None
        self.bias = None

    def build(self, in_features, device):
        limit = (6.0 / (in_features + self.units)) ** 0.5
        self.kernel = torch.nn.Parameter(torch.empty(in_features, self.units, device=device).uniform_(-limit, limit),
                                         requires_grad=False)
        if self.use_bias:
            self.bias = torch.nn.Parameter(torch.zeros(self.units, device=device), requires_grad=False)

    def recording(self, x):
        """Does this call record autograd history (grad mode on, and the input or a weight requires grad)?"""
        return torch.is_grad_enabled() and (x.requires_grad or any(w is not None and w.requires_grad for w in (self.kernel, self.bias)))

    def forward(self, x):
        if self.kernel is None:
            with torch.no_grad():
                self.build(x.shape[-1], x.device)
        if self.recording(x):  # torch's GEMM, differentiable
            return torch.addmm(self.bias, x, self.kernel) if self.bias is not None else x @ self.kernel
        return self._forward_infer(x)

    @torch.no_grad()
    def _forward_infer(self, x):
        if ops.dense_supported(x, self.kernel):
            return ops.dense_forward(x, self.kernel, self.bias)
        if self.bias is not None:
            return torch.addmm(self.bias, x, self.kernel)
        return x @ self.kernel

    def product(self, x, residual=None):
        """``x @ kernel`` (+ ``residual``, inside the GEMM: its C operand) WITHOUT the bias -- the start of a layer's sum
        (models/hrnet.py); the bias rides on the first convolution that accumulates into the result."""
        if self.kernel is None:
            with torch.no_grad():
                self.build(x.shape[-1], x.device)
        if self.recording(x):
            return x @ self.kernel if residual is None else residual + x @ self.kernel
        return self._product_infer(x, residual)

    @torch.no_grad()
    def _product_infer(self, x, residual=None):
        if ops.dense_supported(x, self.kernel):
            return ops.dense_forward(x, self.kernel, None, residual)
        if residual is not None:
            return torch.addmm(residual, x, self.kernel)
        return x @ self.kernel


class BaseModel(PlainAttributes, torch.nn.Module):
    """models/base_model.py:10-29.  ``model(data, training=False)`` runs
    transform -> preprocess -> forward -> postprocess -> inv_transform."""

    def __init__(self, name, **kwargs):
        super().__init__()
        self.model_name = name
        self.cfg = Config(kwargs)  # unknown kwargs (ckpt_path, device, ...) end up here, base_model.py:19-21

    @property
    def name(self):
        return self.model_name

    def __call__(self, data, training=True, **kwargs):
        return self.call(data, training=training, **kwargs)

    def call(self, data, training=True, **kwargs):
        d = self.transform(data, training=training, **kwargs)
        x = self.preprocess(d, training=training, **kwargs)
        x = self.run_forward(x, d, training=training, **kwargs)
        x = self.postprocess(x, d, training=training, **kwargs)
        x = self.inv_transform(x, data, training=training, **kwargs)
        return x

    # torch.nn.Module reserves ``forward`` for __call__ dispatch; the reference's stage is named
    # ``forward(prev, data, training)`` (base_model.py:31-33) and subclasses here keep that name.
    def run_forward(self, prev, data, training=True, **kwargs):
        return self.forward(prev, data, training=training, **kwargs)

    def forward(self, prev, data, training=True, **kwargs):
        raise NotImplementedError

    def recording(self):
        """Does a call now record autograd history (grad mode on and some weight requires grad)?  Weights are built with
        requires_grad=False; ``model.requires_grad_(True)`` enables training.  While recording, the models take their unfused,
        out-of-place forms (the fused epilogues and paired launches have no backward).  A batched step (PBFNet.step_batched)
        takes the same forms whether it records or not: the fused forms know nothing of items."""
        if getattr(self, "_batch", None) is not None:
            return True
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def record_lattice_form(self, on=True):
        """Sets ``record_lattice_form`` on every ContinuousConv of the model: while autograd records, the layers between two
        grid_pos lattices then keep the stencil form and take dmcf_lattice_conv_backward (off: every recording layer takes the
        neighbour-list form, the default).  Inference is not affected.  Returns the number of layers set."""
        from ..utils.convolutions import ContinuousConv
        n = 0
        for m in self.modules():
            if isinstance(m, ContinuousConv):
                m.record_lattice_form = bool(on)
                n += 1
        return n

    def record_scatter_form(self, on=True):
        """Sets ``record_scatter_form`` on every ContinuousConv of the model: while autograd records, the layers that gather
        particles onto a grid_pos lattice with 4 or 8 output channels then take dmcf_cconv_scatter_backward on the transposed list
        (off: the neighbour-list backward with its list inversion, the default).  Inference is not affected.  Returns the number
        of layers set."""
        from ..utils.convolutions import ContinuousConv
        n = 0
        for m in self.modules():
            if isinstance(m, ContinuousConv):
                m.record_scatter_form = bool(on)
                n += 1
        return n

    def loss(self, results, data):
        raise NotImplementedError(f"{type(self).__name__} defines no loss")

    def get_optimizer(self, cfg_pipeline):
        """models/pbf_model.py:508-517 of the reference: Adam (epsilon 1e-6) with a piecewise-constant learning rate."""
        from ..utils.tools.losses import get_optimizer
        return get_optimizer(self.parameters(), cfg_pipeline)

    def transform(self, data, training=True, **kwargs):
        return data

    def inv_transform(self, prev, data, training=True, **kwargs):
        return prev

    def preprocess(self, data, training=True, **kwargs):
        return data

    def postprocess(self, prev, data, training=True, **kwargs):
        return prev
