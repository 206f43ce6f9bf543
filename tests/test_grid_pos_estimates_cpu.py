"""ops._grid_count_levels, the table sizing of grid_pos_many from the second call of a rollout on, driven on the host with fake
``count`` and ``read_headers`` callables that follow a script of cell counts: no library is loaded.  Pinned: the capacities asked
for, the order of the calls, the number of header reads and the entry left in ``_GRID_CELLS``.  The same transitions run on the
device in tests/test_gpu_grid_pos_estimates.py."""
import pytest

torch = pytest.importorskip("torch")

N = 3000          # points of the scripted scene: the sparse rule starts above GRID_MIN_CELLS cells
SLOTS = 1 << 15   # what the caller passes for the hashed table
KEY = ("levels", True, 0, 0.1)


class _Script:
    """A two-level call: ``read_headers`` fills cells and sparse of both levels from ``cells``, ``count`` records (level, capacity)."""

    def __init__(self, ops, cells):
        self.ops, self.cells, self.log = ops, list(cells), []
        self.levels = [dict(name=k) for k in range(len(cells))]

    def count(self, lv, capacity):
        lv["capacity"] = capacity
        self.log.append(("count", lv["name"], capacity))

    def read_headers(self):
        self.log.append(("read",))
        for lv, c in zip(self.levels, self.cells):
            lv["cells"], lv["sparse"] = int(c), self.ops._grid_too_sparse(int(c), N)

    def run(self, key=KEY):
        self.ops._grid_count_levels(self.levels, key, self.count, self.read_headers, SLOTS)
        return self.log


@pytest.fixture
def ops(monkeypatch):
    from dmcf_amd import ops
    monkeypatch.setattr(ops, "_GRID_CELLS", {})
    return ops


def test_size_classes_the_sequence_relies_on(ops):
    assert ops._size_class(0) == 65536 == ops._size_class(2197 + 2197 // 4)
    assert ops._size_class(79507 + 79507 // 4) == 131072 == ops._size_class(97336 + 97336 // 4)
    assert ops._size_class(314432 + 314432 // 4) == 393216
    assert not ops._grid_too_sparse(ops.GRID_MIN_CELLS, N) and ops._grid_too_sparse(ops.GRID_MIN_CELLS + 1, N)
    assert ops._grid_too_sparse(int(6e13), N)


def test_rollout_sequence(ops):
    """Level 0 grows, outgrows its table, dissolves into spray (hashed), comes back, empties and fills again; level 1 stays at
    2197 cells and is never counted twice."""
    S = int(6e13)
    R, H = ("read",), -SLOTS
    c0 = lambda cap: ("count", 0, cap)  # noqa: E731
    c1 = lambda cap: ("count", 1, cap)  # noqa: E731
    steps = [
        # cells of level 0, the calls in order, the entry of level 0 afterwards
        (79507, [R, c0(79507), c1(2197), R], 79507),                    # first call: header first, exact tables
        (97336, [c0(131072), c1(65536), R], 97336),                     # the estimate holds: one header read
        (314432, [c0(131072), c1(65536), R, c0(314432), R], 314432),    # outgrown: level 0 again, exact
        (S, [c0(393216), c1(65536), R, c0(H), R], -1),                  # dense -> hashed
        (S, [c0(H), c1(65536), R], -1),                                 # hashed from the start
        (79507, [c0(H), c1(65536), R], 79507),                          # dense again, but this call ran hashed: no recount
        (79507, [c0(131072), c1(65536), R], 79507),                     # ... and is dense in the next
        (0, [c0(131072), c1(65536), R], 0),                             # an empty call
        (79507, [c0(65536), c1(65536), R, c0(79507), R], 79507),        # the estimate of nothing is the smallest class
    ]
    for k, (cells, want, entry) in enumerate(steps):
        s = _Script(ops, [cells, 2197])
        assert s.run() == want, f"step {k + 1}"
        assert s.log.count(R) == (1 if len(want) == 3 else 2), f"step {k + 1}"
        assert ops._GRID_CELLS == {KEY: [entry, 2197]}, f"step {k + 1}"
        assert s.levels[1]["capacity"] == (2197 if k == 0 else 65536)


def test_both_levels_outgrown_are_both_recounted(ops):
    _Script(ops, [100, 100]).run()
    s = _Script(ops, [70000, int(6e13)])
    assert s.run() == [("count", 0, 65536), ("count", 1, 65536), ("read",), ("count", 0, 70000), ("count", 1, -SLOTS), ("read",)]
    assert ops._GRID_CELLS[KEY] == [70000, -1]


def test_estimate_of_another_length_takes_the_exact_path(ops):
    ops._GRID_CELLS[KEY] = [79507, 2197, 343]  # (three levels under a key that now asks for two)
    s = _Script(ops, [97336, 2197])
    assert s.run() == [("read",), ("count", 0, 97336), ("count", 1, 2197), ("read",)]
    assert ops._GRID_CELLS[KEY] == [97336, 2197]
    ops._GRID_CELLS[KEY] = [79507]
    s = _Script(ops, [int(6e13), 2197])
    assert s.run() == [("read",), ("count", 0, -SLOTS), ("count", 1, 2197), ("read",)]
    assert ops._GRID_CELLS[KEY] == [-1, 2197]


def test_at_most_33_keys_and_the_oldest_leaves(ops):
    keys = [("k", i) for i in range(40)]
    for i, key in enumerate(keys):
        _Script(ops, [1000 + i, 2197]).run(key)
        assert len(ops._GRID_CELLS) == min(i + 1, 33)
        assert list(ops._GRID_CELLS) == keys[max(0, i - 32): i + 1]
    assert ops._GRID_CELLS[keys[-1]] == [1039, 2197] and keys[6] not in ops._GRID_CELLS
    # a key that is already held is updated in place; the eviction before it may still drop the oldest
    _Script(ops, [5, 5]).run(keys[20])
    assert ops._GRID_CELLS[keys[20]] == [5, 5] and len(ops._GRID_CELLS) <= 33
