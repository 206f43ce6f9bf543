"""The backward of the scatter form (dmcf_cconv_scatter_backward: dmcf_amd/csrc/cconv_sct_bwd.inc) restated in numpy in the
kernel's order of evaluation, and the bar both tests/test_cconv_scatter_backward_ref_cpu.py and
tests/test_gpu_cconv_scatter_backward.py hold it to, on the cases of tests/cconv_scatter_ref.py.

    T_j[cell][o]   = sum_{pairs p = (i, j)} a_p sum_k [cell_k(p) == cell] w_k(p) G[i][o]
    dF[j][c]       = sum_{cell, o} W[cell][c][o] T_j[cell][o]
    dW[cell][c][o] = sum_j f_j[c] T_j[cell][o]

    |gpu - ref| <= 256 * 2^-24 * max(A, 1e-6 max A) + fixed                       element by element

ref, A   cconv_backward_ref.grads on the FORWARD list of the pairs the call really has (c.idx, c.rs: rows cut off by the capacity
         are gone), plain and with abs_mode, on PairWeights with the float32 oracle coordinates; the floor is
         cconv_backward_ref.check's.  This is the bar of DESIGN.md section 4.6 for every backward kernel.
fixed    what the 64-bit fixed-point sums into T_j add, derived as in cconv_scatter_ref's docstring.  The kernel forms b =
         float32(max |G| * max(1, |window_fac|)) = m 2^e (0.5 <= m < 1) on the device and adds every term t (a float32) as
         rint(t * 2^s), 2^s = 2^(46 - e): one rounding of at most half a unit, 2^-s / 2 <= b 2^-46, and a factor 2 for a b that
         crosses a power of two which Bg, the same product in double, does not: at most Bg 2^-45 per term.  T_j[cell][o] takes one
         term per pair of row j that has `cell` among its 8 corners, cnt_j(cell) of them; integer addition adds nothing, and the
         conversion back (one rounding to float32) is inside the float part.  Through the two products:
             dF[j][c]:        (sum_cell cnt_j(cell) sum_o |W[cell][c][o]|) Bg 2^-45
             dW[cell][c][o]:  (sum_j cnt_j(cell) |f_j[c]|) Bg 2^-45  <=  (sum_j n_j |f_j[c]|) Bg 2^-45     (the form used)
         with Bg = max |G| * max(1, |window_fac|) in float64 and n_j the pairs of row j.

Condition every case meets, asserted in the CPU file: on every element the fixed term is at most 1 / 16 of the float part, floor
included.  It is a condition on the cases, not a measurement of the kernel."""
import numpy as np

import cconv_backward_ref as ref
from cconv_backward_ref import EPS, WORST

K_BAR = 256
MAX_SHARE = 1.0 / 16


def grad_out(c):
    """dL/d out of a case: the same on the CPU and on the GPU."""
    return np.random.default_rng(500 + c.seed).normal(size=(c.out_pos.shape[0], c.cout)).astype(np.float32)


def pair_weights(c):
    """The constants of the case's pairs from the float32 oracle coordinates, on the forward list the call really has."""
    return ref.PairWeights(c.out_pos, c.inp_pos, c.idx, c.rs, c.extent, (4, 4, 4), window=c.window, window_fac=c.window_fac, f64=False)


def restate(c, pw, G, dtype=np.float64, a=None, cells=None, keep=None):
    """(dW [4,4,4,cin,cout], dF [n_inp,cin], T [n_inp,64,cout]) in the kernel's order: T_j first, then the two products.
    ``a`` / ``cells`` replace the pair weights / the corner cells, ``keep`` (bool [P]) drops pairs: the seeded faults."""
    a = pw.a if a is None else a
    cells = pw.cells if cells is None else cells
    sel = np.ones(pw.i.shape[0], bool) if keep is None else keep
    n_inp = c.inp_pos.shape[0]
    w = (pw.wts[sel] * a[sel, None]).astype(dtype)
    terms = (w[:, :, None] * G.astype(dtype)[pw.i[sel]][:, None, :]).astype(dtype)
    T = np.zeros((n_inp, 64, c.cout), dtype)
    np.add.at(T, (pw.j[sel][:, None], cells[sel]), terms)
    W = c.filt.reshape(64, c.cin, c.cout).astype(dtype)
    dF = np.einsum("kco,jko->jc", W, T).astype(dtype)
    dW = np.einsum("jc,jko->kco", c.feat.astype(dtype), T).astype(dtype)
    return dW.reshape(4, 4, 4, c.cin, c.cout), dF, T


def fixed_terms(c, pw, G):
    """(fixed part of the bar for dW [cin] broadcast over cells and outputs as [1,1,1,cin,1], for dF [n_inp,cin])."""
    Bg = float(np.abs(G.astype(np.float64)).max()) * max(1.0, abs(float(c.window_fac)))
    n_inp = c.inp_pos.shape[0]
    cnt = np.zeros((n_inp, 64))
    np.add.at(cnt, (pw.j[:, None], pw.cells), 1.0)
    absW = np.abs(c.filt.reshape(64, c.cin, c.cout).astype(np.float64)).sum(-1)  # [64, cin]
    unit = Bg * 2.0 ** -45
    n_j = np.bincount(pw.j, minlength=n_inp).astype(np.float64)
    fixed_f = (cnt @ absW) * unit
    fixed_w = ((n_j[:, None] * np.abs(c.feat.astype(np.float64))).sum(0) * unit).reshape(1, 1, 1, c.cin, 1)
    return fixed_w, fixed_f


class Bar:
    """Reference gradients and the two parts of the bar for one case."""

    def __init__(self, c, G=None):
        self.c = c
        self.G = grad_out(c) if G is None else G
        self.pw = pair_weights(c)
        self.want_w, self.want_f, _ = ref.grads(self.pw, c.filt, c.feat, self.G)
        self.A_w, self.A_f, _ = ref.grads(self.pw, c.filt, c.feat, self.G, abs_mode=True)
        self.fixed_w, self.fixed_f = fixed_terms(c, self.pw, self.G)

    @staticmethod
    def float_part(A, factor=1.0):
        A = factor * A
        return K_BAR * EPS * np.maximum(A, 1e-6 * max(float(A.max()) if A.size else 0.0, 1e-30))

    def shares(self):
        """Worst fixed / float part over the elements of (dW, dF)."""
        return (float(np.max(self.fixed_w / self.float_part(self.A_w))), float(np.max(self.fixed_f / self.float_part(self.A_f))))

    def _check(self, name, got, want, A, fixed, factor):
        bar = self.float_part(A, factor) + fixed
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        ratio = float(np.max(err / bar)) if err.size else 0.0
        WORST[name] = max(WORST.get(name, 0.0), ratio)
        assert np.all(err <= bar), f"{name}: worst err/bar {ratio:.3g} at {np.unravel_index(np.argmax(err / bar), err.shape)}"

    def check(self, name, got_w, got_f, want_w=None, want_f=None, factor=1.0):
        """The assertion of this file's docstring; ``want_*`` / ``factor``: against another implementation at ``factor`` times
        the float part.  Records the worst err / bar under ``name``."""
        if got_w is not None:
            self._check(name + ":filters", got_w, self.want_w if want_w is None else want_w, self.A_w, self.fixed_w, factor)
        if got_f is not None:
            self._check(name + ":features", got_f, self.want_f if want_f is None else want_f, self.A_f, self.fixed_f, factor)

    def within(self, got_w, got_f):
        try:
            self.check("_probe", got_w, got_f)
        except AssertionError:
            return False
        finally:
            WORST.pop("_probe:filters", None)
            WORST.pop("_probe:features", None)
        return True
