"""CPU: tests/cnaref.py, the NumPy reference of compute cna/atom/mdp, on constructed cells whose answers are known from the
lattice: fcc perfect, jittered and with a vacancy, a close-packed stack that is half fcc and half hcp, bcc, and an icosahedron.
The jitter is Gaussian from default_rng(1); no cell has an ambiguous atom (a distance within 1e-9 relative of the cutoff)."""
import numpy as np
import pytest

import cnaref

PER = (1, 1, 1)


@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_fcc(sigma):
    x, h = cnaref.fcc_cell(6, sigma)
    r = cnaref.cna(x, h, PER, cnaref.RC_FCC)
    assert len(x) == 864 and not r["ambiguous"].any()
    assert np.all(r["pattern"] == cnaref.FCC) and np.all(r["neighbours"] == 12)


def test_a_vacancy():
    """the twelve neighbours of the vacancy have 11 neighbours and read `other`; everyone else is fcc"""
    full, h = cnaref.fcc_cell(6)
    x, _ = cnaref.fcc_cell(6, gone=431)
    r = cnaref.cna(x, h, PER, cnaref.RC_FCC)
    assert len(x) == 863 and not r["ambiguous"].any()
    assert cnaref.histogram(r["pattern"]).tolist() == [0, 851, 0, 0, 0, 12]
    d = x - full[431]
    d -= np.rint(d / h[0, 0]) * h[0, 0]
    near = np.abs((d * d).sum(axis=1) - 0.5 * cnaref.A_FCC ** 2) < 1e-6
    assert near.sum() == 12 and np.all(r["pattern"][near] == cnaref.OTHER) and np.all(r["neighbours"][near] == 11)


def test_the_stack_is_half_fcc_and_half_hcp():
    x, h, layer = cnaref.stack_cell()
    assert len(x) == 960 and np.allclose(h.diagonal(), [22.88, 24.77, 28.02], atol=5e-3)
    r = cnaref.cna(x, h, PER, cnaref.RC_FCC)
    assert not r["ambiguous"].any() and np.all(r["neighbours"] == 12)
    assert cnaref.histogram(r["pattern"]).tolist() == [0, 480, 480, 0, 0, 0]
    fcc = (layer >= 1) & (layer <= 6)
    assert np.all(r["pattern"][fcc] == cnaref.FCC) and np.all(r["pattern"][~fcc] == cnaref.HCP)


def test_bcc():
    x, h = cnaref.bcc_cell()
    r = cnaref.cna(x, h, PER, cnaref.RC_BCC)
    assert len(x) == 1024 and not r["ambiguous"].any()
    assert np.all(r["pattern"] == cnaref.BCC) and np.all(r["neighbours"] == 14)
    # at the fcc cutoff the six second neighbours are outside: 8 neighbours, `other`
    assert np.all(cnaref.cna(x, h, PER, 0.95 * cnaref.A_BCC)["pattern"] == cnaref.OTHER)


def test_the_icosahedron():
    """the centre has twelve (5,5,2,2) bonds; a vertex has the centre and five vertices: 6 neighbours, `other`"""
    x, h = cnaref.icosahedron_cell()
    r = cnaref.cna(x, h, PER, cnaref.RC_ICO)
    assert len(x) == 13 and not r["ambiguous"].any()
    assert r["pattern"].tolist() == [cnaref.ICO] + [cnaref.OTHER] * 12 and r["neighbours"].tolist() == [12] + [6] * 12


def test_the_group_and_the_signatures():
    """an atom outside the group reads 0 and is still a neighbour; the signatures of an fcc and an hcp centre, and the empty set"""
    x, h, layer = cnaref.stack_cell()
    member = np.arange(len(x)) % 5 != 4
    r = cnaref.cna(x, h, PER, cnaref.RC_FCC, member)
    assert np.all(r["pattern"][~member] == 0) and np.all(r["pattern"][member] > 0) and np.all(r["neighbours"] == 12)
    assert cnaref.histogram(r["pattern"]).tolist() == [192, 384, 384, 0, 0, 0]
    adj = np.zeros((3, 3), dtype=bool)
    adj[0, 1] = adj[1, 0] = True
    assert cnaref.signature(adj, 2) == (0, 0, 0, 8) and cnaref.signature(adj, 0) == (1, 0, 0, 0)
    assert cnaref.pattern_of([(4, 2, 2, 0)] * 12) == cnaref.OTHER       # twelve hcp-like bonds are no hcp
    assert cnaref.pattern_of([(4, 2, 1, 1)] * 6 + [(4, 2, 2, 0)] * 6) == cnaref.HCP


def test_an_edge_distance_is_flagged():
    """a cutoff a rounding away from the second-neighbour distance of the perfect lattice: every atom is ambiguous"""
    x, h = cnaref.fcc_cell(4)
    r = cnaref.cna(x, h, PER, cnaref.A_FCC * (1.0 + 1e-12))
    assert r["ambiguous"].all()
    r = cnaref.cna(x, h, PER, cnaref.RC_FCC)
    assert not r["ambiguous"].any() and np.all(r["pattern"] == cnaref.FCC)
