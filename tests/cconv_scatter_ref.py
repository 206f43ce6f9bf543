"""The scatter form of CConv (splat S, dmcf_cconv_scatter_forward: dmcf_amd/csrc/cconv_sct.hip) against the float64 reference of
tests/cconv_forward_ref.py, element by element, and the deterministic cases both tests/test_cconv_scatter_ref_cpu.py (the bar is
sound, seeded faults break it) and tests/test_gpu_cconv_scatter_bar.py (the kernel) run.

    |gpu - ref| <= (kbar * A + C_GEO * A1) * 2^-24 + n_i * B * 2^-45          element by element

ref, A, A1, kbar, C_GEO   exactly those of cconv_forward_ref (forward_bar / kbar_of on PairWeights(f64=True) of the FORWARD list of
     the pairs the call really has; poly6 formed from the positions, as the kernel forms it), with the floor of
     cconv_backward_ref.check on that float part.
n_i  the number of pairs of output row i.
B    cin * max |f| * max |W| * max(1, |window_fac|), in float64 from the inputs.

The last term is what the 64-bit fixed-point sums add, derived and not measured.  The kernel forms b = float32(cin * max |f|) *
max |W| * max(1, |window_fac|) on the device, writes b = m 2^e with 0.5 <= m < 1, and adds every pair's term c (a float32) as the
integer rint(c * 2^s), 2^s = 2^(46 - e): 2^45 <= 2^s b < 2^46.  One rounding per pair, of at most half a unit: 2^-s / 2 =
2^(e - 47) <= b 2^-46 (b >= 2^(e - 1)).  b itself is a float32 product of three factors (two roundings, 1 + 2^-23 together) and may
cross a power of two that B, the same product in double, does not: then e is one more than B's and the unit is twice as coarse.
One factor of 2 covers that: at most B 2^-45 per pair, n_i B 2^-45 per element.  Integer addition adds no error, and the one
conversion back (the sum times 2^-s as a double, rounded to float32) is a relative 2^-24 of the result, inside kbar * A.

Conditions every case meets, asserted in the CPU file so that no GPU test can hide a failure behind the bar: on every element
the fixed-point term is at most 1 / 16 of the float part (floor included); every n_i < 2^16, the headroom of the 64-bit sums (the
longest row of these cases has a few hundred pairs: nothing here goes near it); no row is left out of the comparison.

The geometry is built on the CPU without the GPU search or grid_pos, in units of lattice cells relative to out[0], the plan's
origin: out = float32(centre + cell * voxel).  The forward list is the oracle's brute-force search; the transposed list is
derived from its pairs by a stable argsort by input index, so both hold the same pairs by construction.

Sizes: about 370 particles and 1000 - 1700 lattice points per case (14 - 35 thousand pairs), the smallest at which a block still
takes three 32-row chunks, a transposed row five 64-pair batches, and several blocks flush into one output point.
"""
import numpy as np

import oracle
import cconv_backward_ref as ref
import cconv_forward_ref as fr
from cconv_backward_ref import EPS, WORST, PairWeights  # noqa: F401

FIXED_BITS = 46
MAX_SHARE = 1.0 / 16   # of the float part of the bar, for the fixed-point term
PITCH = 16             # cells between two sites: a multiple of every block size, wider than a block plus two reaches
# (voxel, radius): R / voxel about 1.7, 2.6 and 4.0, and the 0.4 / 0.1 of Liquid3d's coarsest lattice
KINDS = {"r2": (0.1, 0.17, 2), "r3": (0.1, 0.26, 3), "r4": (0.125, 0.5, 4), "r4x": (0.1, 0.4, 4)}
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 257)  # of a transposed row: the edges of the 64-pair batches
POPULATIONS = (1, 8, 9, 15, 16, 17, 31, 32, 33, 65)       # of a block: the edges of the 16- and 32-row chunks and the double buffer
CINS = (1, 3, 4, 5, 16, 17, 24, 31, 32)
N_BULK = 120
STRAY_SITES = ((700, 0, 0), (0, -640, 16), (-592, -608, 320))  # cells from the origin: beyond 128 blocks of 4 cells
EMPTY_CELLS = ((0, 0, 0), (1, 0, 0), (0, 2, 1), (-1, -1, 0), (3, 3, 3))  # the origin's site: no particle within reach


def expected_reach(radius, voxel):
    """dmcf_cconv_scatter_plan's expression, in float32: ceilf(0.5f * extent / voxel - 1e-4f), extent = 2 * radius."""
    extent = np.float32(2.0 * float(radius))
    return int(np.ceil(np.float32(np.float32(np.float32(0.5) * extent) / np.float32(voxel)) - np.float32(1e-4)))


def expected_kernel(cout, block_cells, reach):
    """The instantiation a (cout, block_cells, reach) runs: 16 waves only where a box of 12^3 slots or more leaves no room for
    two workgroups of 8 (cout 4); cout 8 always takes 8."""
    D = block_cells + 2 * reach + 1
    return f"cconv_sct_kernel<{cout}, {16 if cout == 4 and D >= 12 else 8}>"


def two_workgroups(cout, block_cells, reach):
    """Do two workgroups of 8 waves fit a CU's 160 KB (sct_lds_bytes)?"""
    ns = ((block_cells + 2 * reach + 1) ** 3 + 3) & ~3
    return 2 * (cout * ns * 8 + ns * 4 + 2 * 2 * 8 * 64 * cout * 4 + 16) <= 160 * 1024


def _cube(lo, hi):
    ax = np.arange(lo, hi + 1)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


def _unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


class Scene:
    """Cells (integers, relative to out[0]) and particles (cell units) of one case.  ``probes``: transposed row length -> index
    of the particle whose row has it; ``single`` / ``edge``: (particle, cell) of the lone pair at R / 2 and of the pair at
    0.9995 R; ``populations``: block population -> the block's first cell; ``outlier``: the particle with the large features."""

    def __init__(self, kind, m, interior, strays, outlier, seed):
        rng = np.random.default_rng(7000 + seed)
        ratio = KINDS[kind][1] / KINDS[kind][0]
        k = KINDS[kind][2]
        grid = [(x, y, z) for z in range(2) for y in range(5) for x in range(5)]
        shift = np.asarray((2, 2, 1) if interior else (0, 0, 0))
        sites = [np.asarray(g) - shift for g in grid if tuple(np.asarray(g) - shift) != (0, 0, 0)]
        sites = [sites[t] * PITCH for t in rng.permutation(len(sites))]
        cells, parts = [np.asarray(EMPTY_CELLS)], []
        self.probes, self.populations = {}, {}
        n_part = 0

        def add(c, p):
            nonlocal n_part
            cells.append(np.asarray(c, dtype=np.int64).reshape(-1, 3))
            p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
            parts.append(p)
            n_part += p.shape[0]
            return n_part - p.shape[0]

        near = _cube(-3, 8)  # every cell a particle in [1.5, 3.5)^3 can reach at 4 cells, and more
        # transposed rows of a chosen length: the L cells nearest to the probe are there, the rest of its ball is not
        for L in ROW_LENGTHS:
            if L in (1, 2):
                continue
            anchor = sites.pop()
            for _ in range(400):
                g = rng.uniform(2.0, 3.0, size=3)
                d = np.linalg.norm(near - g, axis=1)
                if (d < ratio * (1 - 1e-3)).sum() > L:
                    break
            if (d < ratio * (1 - 1e-3)).sum() <= L:
                continue  # (a ball of this reach holds fewer cells)
            self.probes[L] = add(anchor + near[np.argsort(d, kind="stable")[:L]], anchor + g)
        # one pair at R / 2
        anchor, c = sites.pop(), np.asarray((2, 2, 2))
        self.probes[1] = add(anchor + c, anchor + c + _unit(rng) * 0.5 * ratio)
        self.single = (self.probes[1], anchor + c)
        # two pairs: one at the window's edge, one near R / 2
        anchor = sites.pop()
        g = c + _unit(rng) * 0.9995 * ratio
        d = np.linalg.norm(near - g, axis=1)
        other = near[np.argmin(np.abs(d - 0.5 * ratio))]
        assert not np.array_equal(other, c)
        self.probes[2] = add(anchor + np.stack([c, other]), anchor + g)
        self.edge = (self.probes[2], anchor + c)
        # blocks of a chosen population: that many particles inside one block's cells, none in its neighbours; a sparse set of
        # the cells they reach
        box = _cube(-k - 1, m + k)
        for n in POPULATIONS:
            anchor = sites.pop()
            p = anchor + rng.uniform(0.05, m - 0.05, size=(n, 3))
            reach = box[np.min(np.linalg.norm(box[:, None, :] - (p - anchor)[None], axis=2), axis=1) < ratio * 0.98]
            add(anchor + reach[rng.permutation(reach.shape[0])[:45]], p)
            self.populations[n] = anchor
        # a jittered bulk over several blocks, every cell present: long output rows that many blocks flush into
        anchor = sites.pop()
        shell = _cube(-3, 8)
        inner = np.all((shell >= 0) & (shell < 6), axis=1)
        shell = shell[~inner][rng.permutation((~inner).sum())[:80]]
        add(anchor + np.concatenate([_cube(0, 5), shell]), anchor + rng.uniform(-0.5, 6.5, size=(N_BULK, 3)))
        self.outlier = None
        if outlier:  # reaches only a few lattice points
            anchor = sites.pop()
            g = rng.uniform(2.0, 3.0, size=3)
            self.outlier = add(anchor + near[np.argsort(np.linalg.norm(near - g, axis=1), kind="stable")[:3]], anchor + g)
        self.strays = []
        if strays:  # far beyond the plan's region of 128 blocks, lattice points around them
            for s in STRAY_SITES:
                s = np.asarray(s)
                p = s + rng.uniform(2.0, 3.0, size=(2, 3))
                d = np.min(np.linalg.norm(near[:, None, :] - (p - s)[None], axis=2), axis=1)
                reach = near[d < ratio * 0.98]
                self.strays.append(add(s + reach[rng.permutation(reach.shape[0])[:40]], p))
        cells = np.concatenate(cells)
        assert np.unique(cells, axis=0).shape[0] == cells.shape[0]
        order = np.concatenate([[0], 1 + rng.permutation(cells.shape[0] - 1)])  # (out[0] stays the origin)
        self.cells = cells[order]
        self.empty_rows = np.flatnonzero(order < len(EMPTY_CELLS))
        parts = np.concatenate(parts)
        perm = rng.permutation(parts.shape[0])
        self.parts = parts[perm]
        where = np.argsort(perm)
        self.probes = {L: int(where[j]) for L, j in self.probes.items()}
        self.single = (int(where[self.single[0]]), self.single[1])
        self.edge = (int(where[self.edge[0]]), self.edge[1])
        self.outlier = None if self.outlier is None else int(where[self.outlier])
        self.strays = [int(where[j]) for j in self.strays] + [int(where[j + 1]) for j in self.strays]


def transpose(idx, rs, n_inp):
    """The forward list's pairs by input point: (t_index int32 [P] of output rows, t_row_splits int64 [n_inp + 1])."""
    i = np.repeat(np.arange(rs.shape[0] - 1), np.diff(rs))
    order = np.argsort(idx, kind="stable")
    t_rs = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_inp))]).astype(np.int64)
    return i[order].astype(np.int32), t_rs


def scale_bits(feat, filt, cin, window_fac):
    """e of the kernel's bound b = m 2^e, formed in float32 as sct_bound_kernel and sct_scale form it."""
    b = np.float32(np.float32(cin) * np.abs(feat).max()) * np.abs(filt).max() * np.float32(max(1.0, abs(float(window_fac))))
    assert b.dtype == np.float32 and b > 0
    return int(np.frexp(b)[1])


class Case:
    """One call: its arrays (numpy), lists, options and bar.  ``spec`` keys: kind (KINDS), m (block_cells), cout, cin, window
    (None | 'poly6'), window_fac, bias, accumulate, form ('csr' | 'padded' | 'cut': the padded list's buffer ends before its last
    rows), interior (out[0] is an interior cell), offset, strays, outlier, zero_channel, seed."""

    DEFAULTS = dict(kind="r4", m=4, cout=4, cin=24, window="poly6", window_fac=1.0, bias=False, accumulate=False, form="csr",
                    interior=True, offset=0.0, strays=False, outlier=False, zero_channel=None, seed=1)

    def __init__(self, **spec):
        s = dict(self.DEFAULTS)
        s.update(spec)
        self.spec = s
        self.__dict__.update(s)
        self.voxel, radius, self.reach = KINDS[self.kind]
        self.radius = float(np.float32(radius))
        self.extent = float(np.float32(2) * np.float32(radius))
        sc = self.scene = Scene(self.kind, self.m, self.interior, self.strays, self.outlier, self.seed)
        rng = np.random.default_rng(9000 + self.seed)
        centre = rng.uniform(-0.5, 0.5, size=3) + self.offset
        self.out_pos = (centre + sc.cells * self.voxel).astype(np.float32)
        self.inp_pos = (centre + sc.parts * self.voxel).astype(np.float32)
        n_inp, n_out = self.inp_pos.shape[0], self.out_pos.shape[0]
        cin, cout = self.cin, self.cout
        self.feat = rng.normal(size=(n_inp, cin)).astype(np.float32)
        if sc.outlier is not None:
            self.feat[sc.outlier] *= np.float32(2.0 ** 10)
        self.filt = rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32)
        if self.zero_channel is not None:
            self.filt[..., self.zero_channel] = 0
        self.bias_v = rng.normal(size=cout).astype(np.float32) if self.bias else None
        self.prior = rng.normal(size=(n_out, cout)).astype(np.float32) if self.accumulate else None
        # the lists: forward (brute force), transposed from the same pairs as CSR and as padded rows
        idx, rs, _ = oracle.fixed_radius_search(self.inp_pos, self.out_pos, self.radius, bruteforce=True)
        self.full_idx, self.full_rs = idx, rs
        self.t_idx, self.t_rs = transpose(idx, rs, n_inp)
        self.t_counts = np.diff(self.t_rs)
        self.cut = 0
        self.p_idx, self.p_begin, _, self.p_cnt = fr.padded_list(self.t_idx, self.t_rs, np.zeros(self.t_idx.shape[0], np.float32), 0)
        if self.form == "cut":
            # the buffer ends ONE entry into the last row of two pairs or more that has two rows behind it: that row begins
            # inside the buffer and reaches past its end (begin + count > capacity), the rows behind it begin past the end
            first = int(np.flatnonzero(self.t_counts[:n_inp - 2] >= 2)[-1])
            self.cut = n_inp - first
            self.p_idx = self.p_idx[:int(self.p_begin[first]) + 1]
        gone = self.p_begin[:-1] + self.p_cnt > self.p_idx.shape[0]  # rows reaching past the buffer count as empty
        assert (gone & (self.p_cnt > 0)).sum() == (self.t_counts[n_inp - self.cut:] > 0).sum() if self.cut else not gone.any()
        self.cut_rows = gone & (self.p_cnt > 0)
        keep = ~gone[idx]
        i = np.repeat(np.arange(n_out), np.diff(rs))[keep]
        self.idx = idx[keep]
        self.rs = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n_out))]).astype(np.int64)
        self.n_pairs = np.diff(self.rs)
        self.pw = PairWeights(self.out_pos, self.inp_pos, self.idx, self.rs, self.extent, (4, 4, 4), window=self.window,
                              window_fac=self.window_fac, nval=None, f64=True)
        self.B = (float(cin) * float(np.abs(self.feat).max()) * float(np.abs(self.filt).max()) *
                  max(1.0, abs(float(self.window_fac))))
        self.kernel = expected_kernel(cout, self.m, self.reach)
        self._bar = None

    def transposed(self):
        """(t_index, t_row_begin, t_row_count or None) as the call takes them."""
        if self.form == "csr":
            return self.t_idx, self.t_rs, None
        return self.p_idx, self.p_begin, self.p_cnt

    def bar(self):
        """(ref, float part of the bar without 2^-24 and before its floor, fixed-point part) [n_out, cout] float64."""
        if self._bar is None:
            want, A, A1 = fr.forward_bar(self.pw, self.filt, self.feat, window=self.window, window_fac=self.window_fac)
            if self.bias_v is not None:
                want, A = want + self.bias_v, A + np.abs(self.bias_v)
            if self.prior is not None:
                want, A = want + self.prior, A + np.abs(self.prior)
            bound = fr.kbar_of(self.pw, self.cin) * A + fr.C_GEO * A1
            fixed = (self.n_pairs[:, None] * self.B * 2.0 ** -(FIXED_BITS - 1)) * np.ones_like(A)
            self._bar = (want, bound, fixed)
        return self._bar

    def float_bar(self):
        """The float part with its floor (cconv_backward_ref.check's): 2^-24 * max(bound, 1e-6 of the largest bound)."""
        bound = self.bar()[1]
        return EPS * np.maximum(bound, 1e-6 * max(float(bound.max()), 1e-30))

    def exact_rows_value(self):
        """What a row without pairs, and a channel with a zero filter slice, must hold exactly: bias, or prior + bias."""
        v = np.zeros((self.out_pos.shape[0], self.cout), np.float32)
        if self.bias_v is not None:
            v = v + self.bias_v
        if self.prior is not None:
            v = self.prior + v
        return v.astype(np.float32)

    def oracle32(self, idx=None, rs=None, bias_rows=None):
        """The float32 CPU oracle on the forward list (+ bias + prior).  ``idx, rs`` replace the list, ``bias_rows`` (bool
        [n_out]) the rows that get the bias (the seeded faults)."""
        if idx is None:
            idx, rs = self.idx, self.rs
        nimp = None
        if self.window is not None:
            row = np.repeat(np.arange(rs.shape[0] - 1), np.diff(rs))
            rel = self.inp_pos[idx] - self.out_pos[row]
            d2 = (rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2]
            r = np.float32(0.5) * np.float32(self.extent)
            nimp = oracle.window(self.window, d2 / (r * r), self.window_fac)
        y = oracle.continuous_conv(self.filt, self.out_pos, self.extent, self.inp_pos, self.feat, idx, rs, nimp)
        if self.bias_v is not None:
            y = y + (self.bias_v if bias_rows is None else np.where(bias_rows[:, None], self.bias_v, np.float32(0)))
        if self.prior is not None:
            y = y + self.prior
        return y.astype(np.float32)

    def pair_terms(self):
        """[P, cout] float64: what each pair adds, a_p * sum_k w_k (f_j . W[cell_k]) -- the kernel's order, G_j first."""
        G = np.einsum("jc,kco->jko", self.feat.astype(np.float64), self.filt.reshape(64, self.cin, self.cout).astype(np.float64))
        t = np.zeros((self.pw.i.shape[0], self.cout))
        for k in range(8):
            t += self.pw.wts[:, k, None] * G[self.pw.j, self.pw.cells[:, k]]
        return t * self.pw.a[:, None]

    def fixed_point_emulation(self, bits=FIXED_BITS):
        """The kernel's sum in numpy: every pair's float64 term rounded to a multiple of 2^-s (2^s b <= 2^bits), added as
        integers, times 2^-s as a double, rounded to float32; + bias, + prior in float32 as cconv_sct_finish adds them."""
        s = bits - scale_bits(self.feat, self.filt, self.cin, self.window_fac)
        q = np.rint(np.ldexp(self.pair_terms(), s)).astype(np.int64)
        acc = np.zeros((self.out_pos.shape[0], self.cout), np.int64)
        np.add.at(acc, self.pw.i, q)
        v = np.ldexp(acc.astype(np.float64), -s).astype(np.float32)
        if self.bias_v is not None:
            v = v + self.bias_v
        if self.prior is not None:
            v = self.prior + v
        return v.astype(np.float32)

    def __repr__(self):
        return ",".join(f"{k}={v}" for k, v in self.spec.items() if self.DEFAULTS[k] != v)


def check(name, got, c, fixed_term=True):
    """The assertion of this file's docstring on case ``c``; records the worst err / bar under ``name``."""
    want, _, fixed = c.bar()
    bar = c.float_bar() + (fixed if fixed_term else 0.0)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = float(np.max(err / bar)) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    assert np.all(err <= bar), f"{name}: worst err/bar {ratio:.3g} at {np.unravel_index(np.argmax(err / bar), err.shape)}"


def within_bar(got, c, fixed_term=True):
    try:
        check("_probe", got, c, fixed_term)
    except AssertionError:
        return False
    finally:
        WORST.pop("_probe", None)
    return True


# ---- the cases --------------------------------------------------------------------------------------------------------------------

# (cout, block_cells, kind): <4, 8> with boxes of 6^3 .. 11^3, <4, 16> with 13^3, <8, 8> with two workgroups per CU (6^3) and one
VARIANTS = ((4, 4, "r4x"), (4, 2, "r4"), (8, 2, "r4x"), (8, 1, "r2"), (4, 1, "r4x"), (4, 4, "r3"), (8, 4, "r3"), (4, 4, "r2"),
            (4, 4, "r4"), (8, 1, "r4"), (4, 2, "r3"))
FORMS = ("csr", "padded", "cut", "csr", "padded")


def matrix():
    """[(id, spec)]: every case of the GPU file."""
    out = []
    for t in range(3 * len(CINS)):
        cout, m, kind = VARIANTS[t % len(VARIANTS)]
        out.append(dict(kind=kind, m=m, cout=cout, cin=CINS[t % len(CINS)], window=None if t % 4 == 2 else "poly6",
                        window_fac=0.5 if t % 4 == 1 else 1.0, bias=t % 2 == 0, accumulate=(t // 3) % 2 == 1, form=FORMS[t % len(FORMS)],
                        interior=t % 7 != 3, seed=1 + t % 3))
    # the outlier (poly6: the pair at the window's edge is the small term next to it), strays, the offset, a zero filter slice
    out += [dict(kind="r4x", m=4, cout=4, cin=24, outlier=True, bias=True),
            dict(kind="r4", m=2, cout=8, cin=17, outlier=True, form="padded", accumulate=True, seed=2),
            dict(kind="r4x", m=4, cout=4, cin=24, strays=True, bias=True, window_fac=0.5),
            dict(kind="r3", m=2, cout=8, cin=5, strays=True, form="cut", window=None, seed=3),
            dict(kind="r4x", m=2, cout=4, cin=16, strays=True, form="padded", window_fac=0.5, accumulate=True, seed=2),
            dict(kind="r4x", m=4, cout=4, cin=24, offset=60.0, bias=True),
            dict(kind="r2", m=1, cout=8, cin=3, offset=60.0, form="cut", seed=2),
            dict(kind="r4x", m=4, cout=4, cin=31, zero_channel=2, bias=True, form="padded"),
            dict(kind="r3", m=4, cout=8, cin=4, zero_channel=7, bias=True, accumulate=True, seed=3),
            dict(kind="r4", m=4, cout=4, cin=32, zero_channel=0, window=None, form="cut", seed=2),
            dict(kind="r4x", m=4, cout=4, cin=1, interior=False, form="cut", bias=True, seed=3),
            dict(kind="r2", m=1, cout=8, cin=32, bias=True, accumulate=True, window_fac=0.5),
            dict(kind="r4x", m=2, cout=8, cin=24, form="cut", bias=True, seed=3)]
    return [(f"{n}-c{s['cin']}o{s['cout']}m{s['m']}{s['kind']}-{s.get('form', 'csr')}", s) for n, s in enumerate(out)]


# the case of the bit-identity tests (no accumulate: the three block sizes run it, and with them 8 and 16 waves) and of the faults
IDENTITY = dict(kind="r4x", m=4, cout=4, cin=24, bias=True)
OUTLIER = dict(kind="r4x", m=4, cout=4, cin=24, outlier=True, bias=True)
