"""The heat current of LAMMPS' compute heat/flux (fed ke/atom, pe/atom and stress/atom NULL virial) in NumPy, as the
reference of mdp_heatflux_sums / compute heatflux/mdp:

    J = sum_i (ke_i + pe_i) v_i + sum_i W_i . v_i,      ke_i = 1/2 mvv2e m_i v_i . v_i

W_i is the symmetric tensor of vatom in LAMMPS order (xx yy zz xy xz yz).  Every component is summed with math.fsum (the
correctly rounded sum of the terms as doubles), and the sum of the terms' magnitudes comes along: a device sum in a fixed
order differs from the exact one by a few ulp of that, which is what the tests bound."""
import math

import numpy as np


def terms(mass, v, eatom, vatom, mvv2e):
    """(conv[n][3], virial[n][3], energy[n]): the per-atom terms (ke + pe) v, W . v and ke + pe"""
    m = np.asarray(mass, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(vatom, dtype=np.float64)
    en = 0.5 * mvv2e * m * (v * v).sum(axis=1) + np.asarray(eatom, dtype=np.float64)
    conv = en[:, None] * v
    vir = np.stack([w[:, 0] * v[:, 0] + w[:, 3] * v[:, 1] + w[:, 4] * v[:, 2],
                    w[:, 3] * v[:, 0] + w[:, 1] * v[:, 1] + w[:, 5] * v[:, 2],
                    w[:, 4] * v[:, 0] + w[:, 5] * v[:, 1] + w[:, 2] * v[:, 2]], axis=1)
    return conv, vir, en


def sums(mass, v, eatom, vatom, mvv2e, member=None):
    """dict(sums[8], mag[8], vector[6]): sums = [sum (ke + pe) v (3), sum W.v (3), count, sum (ke + pe)] over the members (all
    atoms without a member table), mag the sums of the terms' magnitudes in the same layout, vector LAMMPS' six values
    [conv + virial (3), conv (3)]"""
    conv, vir, en = terms(mass, v, eatom, vatom, mvv2e)
    if member is not None:
        keep = np.asarray(member, dtype=bool)
        conv, vir, en = conv[keep], vir[keep], en[keep]
    cols = [conv[:, 0], conv[:, 1], conv[:, 2], vir[:, 0], vir[:, 1], vir[:, 2], np.ones(len(en)), en]
    s = np.array([math.fsum(c) for c in cols])
    mag = np.array([math.fsum(np.abs(c)) for c in cols])
    return dict(sums=s, mag=mag, vector=np.concatenate([s[0:3] + s[3:6], s[0:3]]))
