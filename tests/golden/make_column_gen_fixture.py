"""Generates tests/golden/column_gen.npz: four small runs of the REFERENCE's 1-D SPH column generator (datasets/column_gen.py,
numpy only), called as DatasetGroup.gen_data calls it (np.random.seed(seed), then gen_data(**section, **dataset keys)) with
the dataset keys of configs/column/hrnet.yml (res 100, gravity -10.0, dt 0.0025):

  a  seed 44, offset 10, pts_cnt [1, 5], 100 frames   free flight, then contact near frame 56
  b  seed 44, pts_cnt [20], 12 frames                 the pressure loop runs to its cap of 10 000 iterations
  c  seed 7, rnd 0.05, min_pts 3, max_pts 8, data_cnt 2, 20 frames   the randint + normal draw path
  d  seed 44, pts_cnt [40], 4 frames                  42 points, the largest shipped scene

Every case runs twice: as it is, and with every fluid particle's initial position moved up by one float32 ulp
(np.nextafter, patched in after SPH1D.setup).  The per-scene maximum |difference| of the two runs' frame arrays is the
reference's own sensitivity to a rounding-level change (``sens_pos`` / ``sens_vel``): tests/test_column_gen_cpu.py and
tests/test_gpu_sph1d.py derive their error bar from it.

Run where the reference tree is available (it is imported by path); everywhere else only the committed .npz is read.  What is
stored is DATA: per scene the frame arrays pos / vel [T, n, 3], box, box_normals, grav [T, 3], the number of pressure
iterations of every step (the compute_pres calls), and the two sensitivities -- no reference source.  A few minutes of CPU."""
import importlib.util
import os

import numpy as np

REF = "/root/reference/datasets/column_gen.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "column_gen.npz")
DATASET = dict(res=100, gravity=-10.0, dt=0.0025)
CASES = {
    "a": (44, dict(offset=10.0, pts_cnt=[1, 5], data_cnt=2, timesteps=100)),
    "b": (44, dict(pts_cnt=[20], data_cnt=1, timesteps=12)),
    "c": (7, dict(rnd=0.05, min_pts=3, max_pts=8, data_cnt=2, timesteps=20)),
    "d": (44, dict(pts_cnt=[40], data_cnt=1, timesteps=4)),
}


def load():
    spec = importlib.util.spec_from_file_location("ref_column_gen", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(mod, seed, section, nudge):
    """One gen_data call -> (scenes, per-step iteration counts in call order)."""
    iters = []
    setup, pres, step = mod.SPH1D.setup, mod.SPH1D.compute_pres, mod.SPH1D.step

    def setup_nudged(self, *a, **k):
        setup(self, *a, **k)
        if nudge:
            x = self.particles[self.bcnt:, 0]
            self.particles[self.bcnt:, 0] = np.nextafter(x, np.float32(np.inf))

    def pres_counted(self, *a, **k):
        iters[-1] += 1
        return pres(self, *a, **k)

    def step_counted(self, *a, **k):
        iters.append(0)
        return step(self, *a, **k)

    mod.SPH1D.setup, mod.SPH1D.compute_pres, mod.SPH1D.step = setup_nudged, pres_counted, step_counted
    try:
        np.random.seed(seed)
        data = mod.gen_data(**section, **DATASET)
    finally:
        mod.SPH1D.setup, mod.SPH1D.compute_pres, mod.SPH1D.step = setup, pres, step
    return data, np.asarray(iters, np.int32)


def stack(scene, key):
    return np.stack([np.asarray(f[key], np.float32) for f in scene])


if __name__ == "__main__":
    mod = load()
    out = {}
    for name, (seed, section) in CASES.items():
        data, iters = run(mod, seed, section, nudge=False)
        moved, _ = run(mod, seed, section, nudge=True)
        T = section["timesteps"]
        out[f"{name}_scenes"] = np.int32(len(data))
        for s, (scene, other) in enumerate(zip(data, moved)):
            k = f"{name}_s{s}_"
            out[k + "pos"], out[k + "vel"] = stack(scene, "pos"), stack(scene, "vel")
            out[k + "grav"] = stack(scene, "grav")
            out[k + "box"] = np.asarray(scene[0]["box"], np.float32)
            out[k + "box_normals"] = np.asarray(scene[0]["box_normals"], np.float32)
            out[k + "iters"] = iters[s * T:(s + 1) * T]
            out[k + "sens_pos"] = np.float64(np.abs(out[k + "pos"].astype(np.float64) - stack(other, "pos")).max())
            out[k + "sens_vel"] = np.float64(np.abs(out[k + "vel"].astype(np.float64) - stack(other, "vel")).max())
            print(name, s, out[k + "pos"].shape, "iters", out[k + "iters"].min(), out[k + "iters"].max(), "sens",
                  out[k + "sens_pos"], out[k + "sens_vel"], flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
