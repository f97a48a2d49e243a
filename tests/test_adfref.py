"""CPU: tests/adfref.py, the NumPy brute force the device's bond-angle histograms are checked against, on inputs whose
answers are known by hand."""
import math

import numpy as np
import pytest

import adfref

BOX = np.diag([40.0, 40.0, 40.0])
FREE = (0, 0, 0)


def _cluster():
    """a centre with four neighbours at distance 1, 2, 1.6 and 2: +x, +y, -x and 60 degrees from +x in the xy plane.  Ordered
    pairs of them: (x, y) 90, (x, -x) 180, (x, d) 60, (y, -x) 90, (y, d) 30, (-x, d) 120, each twice."""
    c = np.array([10.0, 10.0, 10.0])
    d = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [-1.6, 0.0, 0.0], [2.0 * math.cos(math.pi / 3), 2.0 * math.sin(math.pi / 3), 0.0]])
    return np.vstack([c, c + d]), np.array([1, 2, 2, 2, 2])


@pytest.mark.parametrize("ordinate,where", [
    ("degree", {30.0: 2, 60.0: 2, 90.0: 4, 120.0: 2, 180.0: 2}),
    ("radian", {math.pi / 6: 2, math.pi / 3: 2, math.pi / 2: 4, 2 * math.pi / 3: 2, math.pi: 2}),
    ("cosine", {math.cos(math.pi / 6): 2, 0.5: 2, 0.0: 4, -0.5: 2, -1.0: 2}),
])
def test_a_cluster_with_known_angles(ordinate, where):
    """only the type-1 atom is a centre (the others see it at more than one radius but the triple asks for a type-1 centre);
    nbin = 17 keeps every angle of the cluster off a bin edge in all three ordinates; 180 degrees lands in the last bin and
    cos = -1 in the first"""
    x, types = _cluster()
    nbin = 17
    ref = adfref.counts(x, types, BOX, FREE, nbin, ordinate, [(1, 1, 2, 2, 2, 2, 0.0, 2.5, 0.0, 2.5)])
    lo, hi = adfref.RANGE[ordinate]
    want = np.zeros(nbin, dtype=np.int64)
    for u, k in where.items():
        want[min(int((u - lo) * nbin / (hi - lo)), nbin - 1)] += k
    assert ref["hist"][0].tolist() == want.tolist() and ref["hist"].sum() == 12
    assert ref["icount"].tolist() == [1] and ref["n_edge"] == 0 and ref["n_shell_edge"] == 0
    assert np.array_equal(ref["hist"], ref["hist_sure"]) and ref["edge_adjacent"].sum() == 0
    adfref.check_bracket(ref["hist"], ref)


def test_shells_and_types_select_the_neighbours():
    """j from the shell [0, 1.2) (+x only), k from [1.4, 2.5) (+y, -x, d): the ordered pairs (x, y) 90, (x, -x) 180, (x, d)
    60, once each; swapped shells give the same angles; an empty type selection gives nothing but still counts its centre;
    a radius exactly at a neighbour's distance is reported as a shell edge"""
    x, types = _cluster()
    tr = [(1, 1, 2, 2, 2, 2, 0.0, 1.2, 1.4, 2.5), (1, 1, 2, 2, 2, 2, 1.4, 2.5, 0.0, 1.2), (1, 1, 1, 1, 2, 2, 0.0, 2.5, 0.0, 2.5),
          (1, 2, 1, 2, 1, 2, 0.0, 1.2, 0.0, 1.2)]
    ref = adfref.counts(x, types, BOX, FREE, 17, "degree", tr)
    want = np.zeros(17, dtype=np.int64)
    want[[5, 8, 16]] = 1
    assert ref["hist"][0].tolist() == want.tolist() and ref["hist"][1].tolist() == want.tolist()
    assert ref["hist"][2].sum() == 0 and ref["icount"].tolist() == [1, 1, 1, 5]
    # * * * within 1.2: the centre has one neighbour (no angle), the +x atom has one; nobody has two
    assert ref["hist"][3].sum() == 0 and ref["n_shell_edge"] == 0 and ref["n_edge"] == 0
    ref = adfref.counts(x, types, BOX, FREE, 18, "degree", tr)
    want = np.zeros(18, dtype=np.int64)
    want[17] = 1
    # 60 and 90 degrees sit on edges of 18 bins of 10 degrees: both are EDGE angles, 180 in the last bin is not
    assert ref["n_edge"] == 2 + 2 and ref["hist_sure"][0].tolist() == want.tolist() and ref["hist"][0].sum() == 3
    assert ref["edge_adjacent"][0].tolist() == [int(b in (5, 6, 8, 9)) for b in range(18)]
    assert adfref.counts(x, types, BOX, FREE, 18, "degree", [(1, 1, 2, 2, 2, 2, 0.0, 1.6, 0.0, 2.5)])["n_shell_edge"] == 1
    with pytest.raises(AssertionError):
        adfref.check_inputs(ref)


def test_the_perfect_fcc_cell():
    """6 x 6 x 6 fcc, a = 4.045, * * * over the first shell (0 .. 3.5), 25 bins in degrees: 12 neighbours, 132 ordered pairs
    per atom -- 48 at 60, 24 at 90, 48 at 120 and 12 at 180 degrees, which sit at 8.33, 12.5 and 16.67 bins and in the last"""
    a, n = 4.045, 6
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.array([[i, j, k] for i in range(n) for j in range(n) for k in range(n)], dtype=float)
    x = (cells[:, None, :] + base[None, :, :]).reshape(-1, 3) * a
    ref = adfref.counts(x, np.ones(len(x), dtype=int), np.diag([a * n] * 3), (1, 1, 1), 25, "degree", [(1, 1, 1, 1, 1, 1, 0.0, 3.5, 0.0, 3.5)])
    want = np.zeros(25, dtype=np.int64)
    want[[8, 12, 16, 24]] = np.array([48, 24, 48, 12]) * len(x)
    assert len(x) == 864 and ref["hist"][0].tolist() == want.tolist()
    assert ref["icount"].tolist() == [864] and ref["n_edge"] == 0 and ref["n_shell_edge"] == 0 and ref["max_neighbours"] == 12
    arr = adfref.normalise(ref["hist"], ref["icount"], 25, "degree", "centre")
    assert arr[[9, 13, 17, 24], 2].tolist() == [48.0, 72.0, 120.0, 132.0]


def test_the_normalisation_by_hand():
    hist = np.array([[0, 2, 6, 0], [0, 0, 0, 0]])
    icount = np.array([4, 3])
    frac = adfref.normalise(hist, icount, 4, "cosine", "fraction")
    assert frac[:, 0].tolist() == [-0.75, -0.25, 0.25, 0.75]                       # delta = 0.5
    assert frac[:, 1].tolist() == [0.0, 0.5, 1.5, 0.0] and frac[:, 2].tolist() == [0.0, 0.25, 1.0, 1.0]
    assert np.all(frac[:, 3:] == 0.0) and float(frac[:, 1].sum() * 0.5) == 1.0      # it integrates to 1
    per = adfref.normalise(hist, icount, 4, "degree", "centre")
    assert per[:, 0].tolist() == [22.5, 67.5, 112.5, 157.5]
    assert per[:, 1].tolist() == [0.0, 2 / (8 * 45.0), 6 / (8 * 45.0), 0.0] and per[:, 2].tolist() == [0.0, 0.5, 2.0, 2.0]
    rad = adfref.normalise(hist, icount, 4, "radian")
    assert np.allclose(rad[:, 0], (np.arange(4) + 0.5) * math.pi / 4, rtol=1e-15)


def test_an_atoms_own_image_is_a_neighbour():
    """one atom in a box with a 3 A edge along x and an outer radius of 3.5: its images at +3 and -3 are its two
    neighbours, 180 degrees apart, in both orders; a second atom sees the same"""
    h = np.diag([3.0, 40.0, 40.0])
    ref = adfref.counts(np.array([[1.0, 5.0, 5.0]]), np.array([1]), h, (1, 0, 0), 10, "degree", [(1, 1, 1, 1, 1, 1, 0.0, 3.5, 0.0, 3.5)])
    assert ref["hist"][0].tolist() == [0] * 9 + [2] and ref["icount"].tolist() == [1] and ref["max_neighbours"] == 2
    ref = adfref.counts(np.array([[1.0, 5.0, 5.0], [1.0, 25.0, 5.0]]), np.array([1, 1]), h, (1, 0, 0), 10, "cosine",
                        [(1, 1, 1, 1, 1, 1, 0.0, 3.5, 0.0, 3.5)])
    assert ref["hist"][0].tolist() == [4] + [0] * 9
