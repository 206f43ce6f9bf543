"""The free-fall datasets -- the reference's ``datasets/free_fall_gen.py``: a disc (``dim=2``) or ball of grid points falling
under gravity, no boundary.  Closed-form host numpy (float64), no kernel: a scene is ``timesteps + 1`` frames of a few hundred
points."""
import numpy as np


def sample_sphere(r, res, sres, dim=2):
    """:5-16: the points of a regular grid over [0.5, res - 0.5]^dim, int((res - 2) sres) per axis, that lie inside the sphere of
    radius ``r`` about the middle of the domain -> [n, 3] float64 (unused axes 0)."""
    rg = np.linspace(0.5, res - 0.5, int((res - 2) * sres))
    axes = [rg if k < dim else [0.0] for k in range(3)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
    center = [res / 2 if k < dim else 0.0 for k in range(3)]
    return grid[np.linalg.norm(grid - center, axis=-1) < r].reshape(-1, 3)


def step(pos, vel, grav, dt, mode=0):
    """:19-27.  ``mode == 0``: symplectic Euler.  Any other mode is the reference's formula as written,
    ``pos + dt vel + (vel + vel1) / 2`` (the mean velocity is NOT scaled by dt there)."""
    vel1 = vel + dt * np.array([0.0, grav, 0.0])
    if mode == 0:
        return pos + dt * vel1, vel1
    return pos + dt * vel + (vel + vel1) / 2, vel1


def gen_dict(pos, vel, idx, res, grav):
    """:30-50: pos / vel float64 [n, 3], one far-away boundary point with a zero normal, everything / res."""
    return [{"frame_id": t, "scene_id": "sim_%04d" % idx, "grav": np.array([0.0, grav, 0.0]) / res, "pos": pos[t] / res,
             "vel": vel[t] / res, "box": np.ones((1, 3)) * res * 2 / res, "box_normals": np.zeros((1, 3))}
            for t in range(len(pos))]


def gen_data(data_cnt=1, timesteps=100, res=100, dim=2, radius=20, dt=0.01, gravity=-10.0, mode=0):
    """:53-78 -> ``data_cnt`` (identical) scenes of ``timesteps + 1`` frames."""
    gravity *= res
    data = []
    for d in range(data_cnt):
        pos = [sample_sphere(radius, res, 0.5, dim)]
        vel = [np.zeros_like(pos[0])]
        for t in range(timesteps):
            p, v = step(pos[t], vel[t], gravity, dt, mode)
            pos.append(p)
            vel.append(v)
        data.append(gen_dict(pos, vel, d, res, gravity))
    return data
