"""The column datasets -- the reference's ``datasets/column_gen.py`` with its 1-D SPH solver on the GPU:

  draw_states  SPH1D.setup :23-34 and the point-count draws of gen_data :294-303: every random number, on the host, in the
               reference's order (the counts, then one ``normal`` per scene), so a seeded call starts from the reference's bits
  rollout      SPH1D.step :159-186 for all scenes of a call at once: ops.sph1d_rollout (dmcf_sph1d_rollout, one wavefront per
               scene).  There is no host solver: without a GPU this raises
  gen_dict     :188-263  per-frame dicts (the 1-D column along y, fluid top-down, then the boundary; everything / res)
  gen_data     :266-317  the reference's keyword set and defaults
"""
import numpy as np

OBS_WALL_POINTS = 50  # side_walls: four columns of this many points, 0.5 apart


def solver_constants(radius=0.25, mass=1.0, stiffness=20.0, visc=0.1, gravity=-10.0, dt=0.01, obs_size=2):
    """SPH1D.__init__ :6-21 and the defaults of step :159 as the keyword arguments of ops.sph1d_rollout."""
    return dict(h=4 * radius, rest_dens=mass / (radius * 2.0), stiffness=stiffness, visc=visc, gravity=gravity, dt=dt, eps=0.01,
                max_iter=10000, bcnt=obs_size)


def draw_states(data_cnt, min_pts=1, max_pts=28, pts_cnt=None, obs_size=2, rnd=0.0, radius=0.25, mass=1.0, offset=0.0):
    """-> (pts_cnt, [state [n + obs_size, 3] float32 = (position, velocity, mass), boundary points first]) -- the global numpy
    generator is used exactly as gen_data :294-303 and SPH1D.setup :23-34 use it."""
    h = 4 * radius
    if pts_cnt is None:
        if rnd > 0:
            pts_cnt = np.random.randint(min_pts, max_pts + 1, size=data_cnt)
        elif data_cnt <= max_pts - min_pts + 1:
            pts_cnt = np.sort(np.random.choice(np.arange(min_pts, max_pts + 1), size=data_cnt, replace=False))
        else:
            raise NotImplementedError("more scenes than distinct point counts (the reference raises here too)")
    states = []
    for d in range(data_cnt):
        cnt = int(pts_cnt[d])
        p = np.zeros((cnt + obs_size, 3), dtype="float32")
        p[:, 0] = np.arange(cnt + obs_size, dtype="float32") * h * 0.5
        if rnd > 0:
            p[obs_size:, 0] += np.random.normal(scale=rnd, size=cnt) * h
        if offset > 0:
            p[obs_size:, 0] += offset
        p[:, 2] = mass
        states.append(p)
    return pts_cnt, states


def rollout(states, timesteps, **constants):
    """Every scene of ``states`` advanced ``timesteps`` steps in one batch -> per scene the sequence [timesteps, n, 2] float32 of
    (position, velocity) before each step, in state order, and the per-step iteration counts [timesteps]."""
    import torch
    from .. import _lib, ops
    if not states:
        return [], []
    if not torch.cuda.is_available():
        raise _lib.DmcfError("the column generator's SPH solver runs on the GPU only (dmcf_sph1d_rollout): no device found")
    n_tot = [len(s) for s in states]
    batch = np.zeros((len(states), max(n_tot), 3), dtype=np.float32)
    for s, st in enumerate(states):
        batch[s, :len(st)] = st
    seq, _, iters = ops.sph1d_rollout(torch.from_numpy(batch).cuda(), n_tot, timesteps, **constants)
    seq, iters = seq.cpu().numpy(), iters.cpu().numpy()
    return [seq[:, s, :n].copy() for s, n in enumerate(n_tot)], [iters[:, s].copy() for s in range(len(states))]


def _across(width):
    """The x offsets of a column drawn ``width`` points wide: [1, width, 3]."""
    x = np.linspace(-(width - 1) * 0.25, (width - 1) * 0.25, width)
    return np.stack([x, np.zeros((width, )), np.zeros((width, ))], axis=-1).reshape(1, width, 3)


def gen_dict(data, idx, res, obs_size, grav, width=1, side_walls=False):
    """:188-263.  ``data``: [T, n + obs_size, 2] (position, velocity), the ``obs_size`` boundary points LAST.  Keys and dtypes as
    the reference's: pos / vel / box / box_normals float32 [., 3] (pos and box float64 when ``width > 1``, where the reference
    adds a float64 linspace), grav float64 [3], frame_id int, scene_id 'sim_%04d'."""
    frames = []
    for t in range(len(data)):
        y, vy, by = data[t, :-obs_size, 0], data[t, :-obs_size, 1], data[t, -obs_size:, 0]
        zero, bzero = np.zeros_like(y), np.zeros_like(by)
        pos = np.stack([zero, y, zero], axis=-1)
        vel = np.stack([zero, vy, zero], axis=-1)
        box = np.stack([bzero, by, bzero], axis=-1)
        normals = np.stack([bzero, bzero + 1, bzero], axis=-1)
        if width > 1:
            pos = (np.expand_dims(pos, axis=1) + _across(width)).reshape(-1, 3)
            box = (np.expand_dims(box, axis=1) + _across(width)).reshape(-1, 3)
            vel = np.repeat(vel, width, axis=0)
            normals = np.repeat(normals, width, axis=0)
            if side_walls:
                z = np.zeros(OBS_WALL_POINTS)
                p = np.arange(OBS_WALL_POINTS, dtype="float32") * 0.5
                edge = (width + 1) * 0.25
                box = np.concatenate([box] + [np.stack([z + x, p, z], axis=-1) for x in (-edge, -edge - 0.5, edge, edge + 0.5)],
                                     axis=0)
                normals = np.concatenate([normals] + [np.stack([z + s, z, z], axis=-1) for s in (1, 1, -1, -1)], axis=0)
        pos /= res
        vel /= res
        box /= res
        frames.append({"frame_id": t, "scene_id": "sim_%04d" % idx, "grav": np.array([0.0, grav, 0.0]) / res, "pos": pos,
                       "vel": vel, "box": box, "box_normals": normals})
    return frames


def gen_data(data_cnt, timesteps, res=100, min_pts=1, max_pts=28, pts_cnt=None, obs_size=2, dt=0.01, rnd=0.0, radius=0.25,
             mass=1.0, stiffness=20.0, visc=0.1, width=1, gravity=-10.0, side_walls=False, offset=0.0):
    """:266-317 -> a list of ``data_cnt`` scenes, each a list of ``timesteps`` frame dicts.  Scenes over 62 fluid points
    (64 with the boundary) raise NotImplementedError (ops.sph1d_rollout)."""
    gravity *= res
    _, states = draw_states(data_cnt, min_pts, max_pts, pts_cnt, obs_size, rnd, radius, mass, offset)
    seqs, _ = rollout(states, timesteps, **solver_constants(radius, mass, stiffness, visc, gravity, dt, obs_size))
    # a frame lists the points top-down: the state reversed, which puts the boundary last (:310-311)
    return [gen_dict(np.ascontiguousarray(seq[:, ::-1]), d, res, obs_size, gravity, width, side_walls) for d, seq in enumerate(seqs)]
