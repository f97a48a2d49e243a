"""CPU: the fixed seeds of the GPU nets (tests/nets.py SUITE, run by tests/test_gpu_nets.py) reach the corners the nets
exist for.  A later trim of the seeds or of the case counts that loses a corner fails here, not silently."""
import random

import numpy as np
import pytest

import nets

SPECS = {net: [s for seed, n in nets.SUITE[net] for s in nets.cases(net, seed, n)] for net in nets.NETS}

CORNERS = {
    "force": {
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "device lists, both styles": lambda c: {s["style"] for s in c if s["lists"] == "device"} == {"rebomos", "aeam"},
        "host CSR lists, both styles": lambda c: {s["style"] for s in c if s["lists"] == "host_csr"} == {"rebomos", "aeam"},
        "a sheared alloy box": lambda c: any(s["style"] == "aeam" and s["tilt"] is not None for s in c),
        "every REBO replica": lambda c: {s["rep"] for s in c if s["style"] == "rebomos"} == {None, (2, 1, 1), (1, 2, 1), (2, 2, 1), (1, 1, 2)},
        "Si fraction 0": lambda c: any(s["style"] == "aeam" and s["frac"] == 0.0 for s in c),
        "Si fraction 0.5": lambda c: any(s["style"] == "aeam" and s["frac"] == 0.5 for s in c),
    },
    "hostmode_walk": {
        "both styles with library-kept images": lambda c: {s["style"] for s in c if s["images"]} == {"rebomos", "aeam"},
        "both styles with host ghosts": lambda c: {s["style"] for s in c if not s["images"]} == {"rebomos", "aeam"},
        "one atom moved far": lambda c: any(m == "one" for s in c for m, _ in s["walk"]),
        "a set inner skin": lambda c: any(s["env"] for s in c),
    },
    "aeam_types": {
        "at most 8 types (tile kernels)": lambda c: any(s["ntypes"] <= 8 for s in c),
        "more than 8 types (generic kernels)": lambda c: any(s["ntypes"] > 8 for s in c),
    },
    "prune": {
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "5 000 K with a drift": lambda c: any(s["temp"] == 5000 and any(s["drift"]) for s in c),
        "MDP_LJ_QUEUE queued and walked": lambda c: any({"queued", "walked"} <= {n for n, _ in s["variants"]} for s in c),
        "other inner skins": lambda c: any({"inner_skin_0.3", "inner_skin_1.2"} <= {n for n, _ in s["variants"]} for s in c),
    },
    "dd": {
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "an odd rank count": lambda c: any(s["ranks"] % 2 for s in c),
        "mid-run thermo steps": lambda c: any(s["thermo"] != s["steps"] for s in c),
    },
    "hnve": {
        "a projectile": lambda c: any(s["shot"] for s in c),
        "no projectile": lambda c: any(not s["shot"] for s in c),
        "both skins": lambda c: {s["skin"] for s in c} == {1.0, 2.0},
    },
    "minilmp": {
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "host mode on several ranks": lambda c: any(s["np"] > 1 for s in c),
        "fix nve/mdp in its one-rank modes": lambda c: any(s["np"] == 1 for s in c),
    },
    "trajectory": {
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "a projectile": lambda c: any(s["shot"] for s in c),
        "a sheared alloy box": lambda c: any(s["style"] == "aeam" and s["tilt"] is not None for s in c),
    },
    "block": {
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
    },
    "fire": {   # (what the iterations of these cases reach: test_fire_cases_reach_their_corners_in_the_reference)
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "delaystep 0": lambda c: any(s["modify"]["delaystep"] == 0 for s in c),
        "halfstepback and initialdelay, each on and off": lambda c: all({s["modify"][k] for s in c} == {True, False}
                                                                         for k in ("halfstepback", "initialdelay")),
        "every degenerate value": lambda c: all(any(s["modify"][k] == v for s in c) for k, v in
                                                 (("dtgrow", 1.0), ("dtshrink", 1.0), ("alphashrink", 1.0), ("tmax", 1.0), ("tmin", 1.0))),
        "every starting time step": lambda c: {s["dt"] for s in c} == {0.001, 0.002, 0.004},
    },
    "langevin": {
        "every path": lambda c: {s["path"] for s in c} == set(nets.LGV_PATHS),
        "both styles on bricks": lambda c: {s["style"] for s in c if s["path"] == "bricks"} == {"rebomos", "aeam"},
        "an odd rank count": lambda c: any(s["ranks"] % 2 and s["ranks"] > 1 for s in c),
        "both styles without the check": lambda c: {s["style"] for s in c if s["path"] == "resident-plain"} == {"rebomos", "aeam"},
        "both styles host-linked": lambda c: {s["style"] for s in c if s["path"] == "hostlinked"} == {"rebomos", "aeam"},
        "a run that crosses step 2^32": lambda c: any(s["first"] < 2 ** 32 < s["first"] + s["nsteps"] for s in c),
        "a run above step 2^32": lambda c: any(s["first"] > 2 ** 32 for s in c),
        "0 K as a target": lambda c: any(s["t1"] == 0.0 for s in c),
        "0 K throughout": lambda c: any(s["t0"] == 0.0 and s["t1"] == 0.0 for s in c),
        "a ramp downwards": lambda c: any(s["t1"] < s["t0"] for s in c),
        "a time step other than 1 fs": lambda c: {s["dt"] for s in c} >= {0.0005, 0.002},
        "zero and tally together": lambda c: any(s["zero"] and s["tally"] for s in c),
        "neither zero nor tally": lambda c: any(not s["zero"] and not s["tally"] and s["path"] != "bricks" for s in c),
        "a ratio on one type only": lambda c: any(s["ratio"] == "one" for s in c),
        "a sheared alloy box": lambda c: any(s["style"] == "aeam" and s["tilt"] is not None for s in c),
        "four fill levels of the last 256-atom block": lambda c: len({s["n"] % 256 for s in c}) >= 4,
        "reads that find the final half deferred, and not": lambda c: {d for s in c for _, d in s["reads"]} == {True, False},
    },
    "heat": {   # (what the reference makes of these cases: test_heat_cases_run_clean_and_the_limits_are_the_references)
        "three sources": lambda c: any(s["nsrc"] == 3 for s in c),
        "four sources": lambda c: any(s["nsrc"] == 4 for s in c),
        "a read step whose due word is neither empty nor full": lambda c: any(0 < nets.heat_due(s, r) < (1 << s["nsrc"]) - 1
                                                                                for s in c for r, _ in s["reads"]),
        "first % nevery != 0 for a source with nevery > 1": lambda c: any(ne > 1 and s["first"] % ne for s in c for ne in s["nevery"]),
        "first = 2^32 + 7": lambda c: any(s["first"] == 2 ** 32 + 7 for s in c),
        "integrate group all": lambda c: any(s["group"] == "all" for s in c),
        "a part of the cell as integrate group": lambda c: any(s["group"] == "slab" for s in c),
        "a tiny group": lambda c: any(q["kind"] == "tiny" for s in c for q in s["shapes"]),
        "a contiguous slab": lambda c: any(q["kind"] == "slab" for s in c for q in s["shapes"]),
        "sources that cover the integrate group": lambda c: any(s["shapes"][-1]["kind"] == "rest" for s in c),
        "a second run from a due step, the first one completed": lambda c: any(
            s["cut"] and s["cut"][1] and any((s["first"] + s["cut"][0]) % ne == 0 for ne in s["nevery"]) for s in c),
        "a second run over a pending final half": lambda c: any(s["cut"] and not s["cut"][1] for s in c),
        "a second run host-linked": lambda c: any(s["cut"] and s["path"] == "hostlinked" for s in c),
        "every path": lambda c: {s["path"] for s in c} == set(nets.HEAT_PATHS),
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "a sheared alloy box": lambda c: any(s["tilt"] is not None for s in c),
        "slot k is not always the k-th lowest bit": lambda c: any(s["bits"] != sorted(s["bits"]) for s in c),
        "at most 16 cases": lambda c: len(c) <= 16,
    },
    "measure": {   # (what the references make of these cases: test_measure_cases_meet_their_own_conditions)
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "a sheared alloy box": lambda c: any(s["tilt"] is not None for s in c),
        "more than 2 types": lambda c: any(s["ntypes"] > 2 for s in c),
        "more than 8 types": lambda c: any(s["ntypes"] > 8 for s in c),
        "a free dimension": lambda c: any(any(s["nonperiodic"]) for s in c),
        "an odd rank count above 1": lambda c: any(s["ranks"] % 2 and s["ranks"] > 1 for s in c),
        "8 ranks": lambda c: any(s["ranks"] == 8 for s in c),
        "half of the cases on one rank, within 4": lambda c: abs(sum(s["ranks"] == 1 for s in c) - len(c) // 2) <= 4,
        "npair = 32": lambda c: any(len(s["pairs"]) == 32 for s in c),
        "ntriple = 32": lambda c: any(len(s["triples"]) == 32 for s in c),
        "nbin = 1, both computes": lambda c: any(s["nbin_rdf"] == 1 for s in c) and any(s["nbin_adf"] == 1 for s in c),
        "nbin x npair = 8192": lambda c: any(s["nbin_rdf"] * len(s["pairs"]) == 8192 for s in c),
        "nbin x ntriple = 8192": lambda c: any(s["nbin_adf"] * len(s["triples"]) == 8192 for s in c),
        "no histogram above 8192 counters": lambda c: all(s["nbin_rdf"] * len(s["pairs"]) <= 8192 and s["nbin_adf"] * len(s["triples"]) <= 8192 for s in c),
        "the cutoff at its limit": lambda c: any(s["cutoff"] is None for s in c),
        "a small cutoff that exceeds the cap of bin_grid at binsize = cutoff / 2": lambda c: any(s["small"] and nets.measure_grid_grows(s) for s in c),
        "each group kind": lambda c: {s["group"]["kind"] for s in c} == set(nets.MSR_GROUPS),
        "every ordinate": lambda c: {s["ordinate"] for s in c} == set(nets.MSR_ORDINATES),
        "MDP_MEASURE_GRID set and unset": lambda c: {s["env"].get("MDP_MEASURE_GRID") for s in c} >= {None, "1"},
        "the device's own check and forced rebuilds": lambda c: {s["rebuild"] == "auto" for s in c} == {True, False},
        "a drift on several ranks": lambda c: any(any(s["drift"]) and s["ranks"] > 1 for s in c),
        "at most 16 cases": lambda c: len(c) <= 16,
    },
    "peratom": {   # (what the reference makes of these cases: test_peratom_cases_meet_their_own_conditions)
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "a box with all three tilts": lambda c: any(s["tilt"] is not None and all(s["tilt"]) for s in c),
        "a free dimension": lambda c: any(any(s["nonperiodic"]) for s in c),
        "8 bricks": lambda c: any(s["ranks"] == 8 for s in c),
        "each group kind": lambda c: {s["group"]["kind"] for s in c} == set(nets.PA_GROUPS),
        "a group of one atom": lambda c: any(s["group"]["kind"] == "few" and len(s["group"]["tags"]) == 1 for s in c),
        "bit 31 on a group with members": lambda c: any(s["group"]["bit"] == 1 << 31 and s["group"]["kind"] not in ("none", "nobody") for s in c),
        "0 K": lambda c: any(s["temp"] == 0 for s in c),
        "819 rows": lambda c: any(nets.peratom_rows(g) == 819 for s in c for g in s["grids"]),
        "820 rows": lambda c: any(nets.peratom_rows(g) == 820 for s in c for g in s["grids"]),
        "a 3-d grid": lambda c: any(len(g[0]) == 3 and min(g[1]) > 1 for s in c for g in s["grids"]),
        "a grid above 4 096 words": lambda c: any(nets.peratom_rows(g) * 5 > 4096 for s in c for g in s["grids"]),
        "every case has a grid in LDS": lambda c: all(min(nets.peratom_rows(g) for g in s["grids"]) * 5 <= 4096 for s in c),
        "no grid above PROFILE_MAXBINS": lambda c: all(nets.peratom_rows(g) <= nets.PA_MAXBINS for s in c for g in s["grids"]),
        "the knob at 1 on one brick": lambda c: any(s["env"].get("MDP_MEASURE_GRID") == "1" and s["ranks"] == 1 for s in c),
        "the knob unset": lambda c: any(not s["env"] for s in c),
        "origins taken mid-run": lambda c: any(s["origin"]["at"] == "between" for s in c),
        "origins from the current positions and by tag": lambda c: {s["origin"]["mode"] for s in c} == {"null", "tag"},
        "a com read of a group": lambda c: any(s["group"]["kind"] not in ("none", "nobody") for s in c),
        "a deferred last half, and not": lambda c: {s["defer"] for s in c} == {True, False},
        "each compute reads first after a deferred half": lambda c: {s["first_read"] for s in c if s["defer"] and (s["heatflux"] or s["first_read"] != "heatflux")} == set(nets.PA_ORDER),
        "a fast drift": lambda c: any(s["fast_on"] for s in c),
        "a drift on several bricks": lambda c: any(any(s["drift"]) and s["ranks"] > 1 for s in c),
        "heatflux on a sheared alloy and on one with a free dimension": lambda c: any(s["heatflux"] and s["tilt"] is not None for s in c)
        and any(s["heatflux"] and any(s["nonperiodic"]) for s in c),
        "the device's own check and forced rebuilds": lambda c: {s["rebuild"] == "auto" for s in c} == {True, False},
        "at most 16 cases": lambda c: len(c) <= 16,
    },
    "structure": {   # (what the references make of these cases: test_structure_cases_meet_their_own_conditions)
        "both styles": lambda c: {s["style"] for s in c if s["cell"] is None} == {"rebomos", "aeam"},
        "each constructed cell": lambda c: {s["cell"] for s in c if s["cell"]} == set(nets.STR_CELLS),
        "a constructed cell on several bricks": lambda c: any(s["cell"] and s["ranks"] > 1 for s in c),
        "an alloy with all three tilts on one brick": lambda c: any(s["tilt"] is not None and all(s["tilt"]) and s["ranks"] == 1 for s in c),
        "an alloy with all three tilts on several bricks": lambda c: any(s["tilt"] is not None and all(s["tilt"]) and s["ranks"] > 1 for s in c),
        "more than 2 types": lambda c: any(s["ntypes"] > 2 for s in c),
        "a free dimension": lambda c: any(any(s["nonperiodic"]) for s in c),
        "8 bricks": lambda c: any(s["ranks"] == 8 for s in c),
        "an odd brick count above 1": lambda c: any(s["ranks"] % 2 and s["ranks"] > 1 for s in c),
        "a drift on several bricks": lambda c: any(any(s["drift"]) and s["ranks"] > 1 for s in c),
        "each group kind": lambda c: {s["group"]["kind"] for s in c} == set(nets.PA_GROUPS),
        "a group of one atom": lambda c: any(s["group"]["kind"] == "few" and len(s["group"]["tags"]) == 1 for s in c),
        "bit 31 on a group with members": lambda c: any(s["group"]["bit"] == 1 << 31 and s["group"]["kind"] not in ("none", "nobody") for s in c),
        "1 column": lambda c: any(len(s["first"]["cols"]) == 1 for s in c),
        "32 columns": lambda c: any(len(s["first"]["cols"]) == 32 for s in c),
        "N = 2": lambda c: any(s["first"]["nnn"] == 2 for s in c),
        "N = 64": lambda c: any(s["first"]["nnn"] == 64 for s in c),
        "centro with the cutoff at the limit": lambda c: any(p["centro_cutoff"] is None for s in c for p in nets.structure_sets(s)),
        "centro's limit capped (MoS2)": lambda c: any(p["centro_capped"] for s in c for p in nets.structure_sets(s)),
        "a coord cutoff small enough that bin_grid widens its cells": lambda c: any(
            p["coord_kind"] == "shell" and nets.measure_grid_grows(s, p["coord_cutoff"]) for s in c for p in nets.structure_sets(s)),
        "every kind of coord cutoff": lambda c: {s["first"]["coord_kind"] for s in c} == set(nets.STR_CUTOFFS),
        "the knob at 1 on one brick": lambda c: any(s["env"].get("MDP_MEASURE_GRID") == "1" and s["ranks"] == 1 for s in c),
        "the knob unset": lambda c: any(not s["env"] for s in c),
        "both kinds of second setup": lambda c: {s["second"] is None for s in c} == {True, False},
        "a second setup with another N and other columns": lambda c: any(
            s["second"] and s["second"]["nnn"] != s["first"]["nnn"] and len(s["second"]["cols"]) != len(s["first"]["cols"]) for s in c),
        "0 K": lambda c: any(s["cell"] is None and s["temp"] == 0 for s in c),
        "the device's own check and forced rebuilds": lambda c: {s["rebuild"] == "auto" for s in c if s["cell"] is None} == {True, False},
        "at most 16 cases": lambda c: len(c) <= 16,
    },
    "postforce": {   # (what the reference makes of these cases: test_postforce_cases_meet_their_own_conditions)
        "every shape x side x dim": lambda c: {(q["shape"], q["side"], q["dim"]) for s in c for q in s["inds"]} >= set(nets.PF_COMBOS),
        "every path": lambda c: {s["path"] for s in c} == set(nets.HEAT_PATHS),
        "both styles": lambda c: {s["style"] for s in c} == {"rebomos", "aeam"},
        "a sheared cell with dynamics and an indenter": lambda c: any(s["tilt"] and s["nsteps"] and s["inds"] for s in c),
        "a sheared cell with dynamics and a spring": lambda c: any(s["tilt"] and s["nsteps"] and s["springs"] for s in c),
        "a sheared cell whose crystal travels along z under a spring": lambda c: any(
            s["tilt"] and s["springs"] and s["springs"][s["drifting"]]["kind"] == "everything" and s["group"] == "all" for s in c),
        "a static case with a free dimension": lambda c: any(s["free"] is not None and s["nsteps"] == 0 for s in c),
        "an indenter with K = 0": lambda c: any(q["k"] == 0.0 for s in c for q in s["inds"]),
        "a spring with K = 0": lambda c: any(q["k"] == 0.0 for s in c for q in s["springs"]),
        "a bit-0 slot behind a slot with a bit": lambda c: any(q["bit"] == 0 and any(p["bit"] for p in s["inds"][:k])
                                                                for s in c for k, q in enumerate(s["inds"])),
        "slot k is not always the k-th lowest bit": lambda c: any([q["bit"] for q in s["inds"]] != sorted(q["bit"] for q in s["inds"]) for s in c),
        "both stages on with 3 or more slots each": lambda c: any(len(s["inds"]) >= 3 and len(s["springs"]) >= 3 for s in c),
        "a spring's group emptied by a new mask": lambda c: any(s["newmask"] for s in c),
        "a second run over a pending final half": lambda c: any(s["cut"] and not s["cut"][1] for s in c),
        "a second run, the first one completed": lambda c: any(s["cut"] and s["cut"][1] for s in c),
        "a second run with both stages on": lambda c: any(s["cut"] and s["inds"] and s["springs"] for s in c),
        "first = 2^32 + 7": lambda c: any(s["first"] == 2 ** 32 + 7 for s in c),
        "256 atoms": lambda c: any(s["n"] == 256 for s in c),
        "288 atoms": lambda c: any(s["n"] == 288 for s in c),
        "more than 1024 atoms, the last 1024-atom block partial": lambda c: any(s["n"] > 1024 and s["n"] % 1024 for s in c),
        "three fill levels of the last 256-atom block": lambda c: len({s["n"] % 256 for s in c}) >= 3,
        "a plane with R = 0": lambda c: any(q["shape"] == "plane" and q["r_plane"] == 0.0 for s in c for q in s["inds"]),
        "a sphere centred on a held atom (r == 0)": lambda c: any(q["site"] == "held" for s in c for q in s["inds"]),
        "static and moving indenters": lambda c: {q["moving"] for s in c if s["nsteps"] for q in s["inds"]} == {True, False},
        "a centre moved by a whole box vector, each dimension": lambda c: {q["shift"][0] for s in c for q in s["inds"]
                                                                           if q["shift"] and q["shape"] != "plane"} == {0, 1, 2},
        "every rest length": lambda c: {q["r0"] for s in c for q in s["springs"]} == {"zero", "below", "above"},
        "static and moving tether points": lambda c: {q["moving"] for s in c for q in s["springs"]} == {True, False},
        "six of the seven use patterns": lambda c: len({q["use"] for s in c for q in s["springs"]}) >= 6,
        "a spring on bit 0": lambda c: any(q["bit"] == 0 for s in c for q in s["springs"]),
        "a tiny group under a spring": lambda c: any(q["kind"] == "tiny" for s in c for q in s["springs"]),
        "start image flags, and none": lambda c: {s["img"] for s in c if s["springs"]} == {True, False},
        "integrate group all, and a part of the cell": lambda c: {s["group"] for s in c} == {"all", "slab"},
        "reads that find the final half deferred, and not": lambda c: {d for s in c for _, d in s["reads"]} == {True, False},
        "at most 16 cases": lambda c: len(c) <= 16,
    },
}


@pytest.mark.parametrize("net,corner", [(n, k) for n in CORNERS for k in CORNERS[n]])
def test_fixed_seeds_reach_the_corner(net, corner):
    assert CORNERS[net][corner](SPECS[net]), f"{net}: no case of {nets.SUITE[net]} reaches '{corner}'"


def test_every_net_has_its_corners_and_at_most_8_ranks():
    assert set(CORNERS) == set(nets.NETS) == set(nets.SUITE)
    assert all(s["ranks"] <= 8 for s in SPECS["dd"]) and all(s["np"] <= 8 for s in SPECS["minilmp"])
    assert all(s["ranks"] <= 8 for s in SPECS["langevin"])
    assert {s["ranks"] for s in SPECS["langevin"] if s["path"] == "bricks"} <= {2, 3, 4, 8}
    assert all(s["ranks"] == 1 for s in SPECS["langevin"] if s["path"] != "bricks")


def test_draws_are_pure_and_repeatable():
    for net in nets.NETS:
        seed, n = nets.SUITE[net][0]
        assert nets.cases(net, seed, n) == nets.cases(net, seed, n)
        assert all(set(s["env"]) <= set(nets.KNOBS) for s in SPECS[net])


def test_draws_reproduce_recorded_cases():
    """first cases of recorded runs of the command-line nets (profiles/r06_*_fuzz/): `profiles/<net>_fuzz.py <cases>
    <seed>` still draws the cases it drew when they were recorded"""
    s = nets.cases("dd", 6, 3)
    assert [(c["style"], c["ranks"], c["rep"], c["temp"], c["drift"], c["steps"], c["seed"]) for c in s] == [
        ("rebomos", 6, (2, 4, 3), 300, [-60, -30, 70], 90, 7889558), ("aeam", 4, (12, 12, 12), 1200, [-30, 70, 25], 90, 9047122),
        ("rebomos", 3, (3, 2, 4), 5000, [70, 70, 0], 90, 1478225)]
    f = nets.cases("force", 11, 1)[0]
    assert f["desc"] == "cells 7 frac 0.08 amp 0.152 seed 615917 tilt [2.07, -0.16, 0.77] lists device"
    m = nets.cases("minilmp", 7, 1)[0]
    assert (m["np"], m["desc"]) == (2, "aeam cells 14 frac 0.0075 T 300 steps 60 seed 8990609")
    h = nets.cases("hnve", 1, 1)[0]
    assert (h["n"], h["temp"], h["skin"], h["shot"], h["seed"], h["env"]) == (576, 300, 2.0, True, 140892, {"MDP_INNER_SKIN": "0.5"})
    t = nets.cases("trajectory", 5, 1)[0]
    assert (t["style"], t["n"], t["temp"], t["shot"], t["seed"]) == ("aeam", 500, 2500, None, 777821)


def test_nvt_seed_reaches_its_corners():
    """the thermostat net of tests/test_gpu_nvt_net.py (nets.NVT_SUITE)"""
    c = nets.nvt_cases(*nets.NVT_SUITE)
    for path in ("resident", "hostlinked"):
        assert any(s["tchain"] == 8 and s["path"] == path for s in c), f"no chain of 8 on the {path} path"
    host = [s for s in c if s["path"] == "hostlinked"]
    assert {s["tloop"] for s in host} >= {2, 3} and any(s["drag"] > 0 for s in host)
    assert {s["tloop"] for s in c} == {1, 2, 3} and {s["drag"] for s in c} == {0.0, 0.2, 0.5}
    assert {s["style"] for s in c} == {"rebomos", "aeam"} and all(s["style"] == "rebomos" for s in host)
    assert any(s["t0"] != s["t1"] for s in c) and any(s["t0"] == s["t1"] for s in c)
    # the last 256-atom block: several fill levels, a full one among them (n % 256 == 1 no cell of either style allows)
    assert len({s["n"] % 256 for s in c}) >= 4 and any(s["n"] % 256 == 0 for s in c)


def test_fire_cases_reach_their_corners_in_the_reference(oracle):
    """Needs the oracle, no GPU: fireref.minimize with ORACLE forces over the suite's `fire` cases (nets.trace_fire).  The
    reference alone must reach what the net exists for -- the device then has to follow it there.  And every case stays a
    minimisation: no atom moves further than the style's skin in its 80 iterations (a run that blows up cannot be held to
    1e-9 eV/A; draw_fire keeps the ceiling of the time step at 10 fs for that reason)."""
    seen, far = {}, 0.0
    for spec in SPECS["fire"]:
        m, dt0 = spec["modify"], spec["dt"]
        dtmax, dtmin = m["tmax"] * dt0, m["tmin"] * dt0
        rows = nets.trace_fire(spec)
        assert len(rows) == spec["niter"] == 80
        far = max(far, rows[-1]["moved"])
        assert rows[-1]["moved"] < {"rebomos": 2.0, "aeam": 1.0}[spec["style"]], (spec["id"], rows[-1]["moved"])
        assert m["tmax"] * dt0 <= 0.0101
        for r in rows:
            held = m["initialdelay"] and r["iter"] < m["delaystep"]
            negative = not r["mixed"]
            hit = {
                "dt == dtmax with tmax < 10": m["tmax"] < 10 and r["dt"] == dtmax and r["dt_before"] * m["dtgrow"] > dtmax,
                "a shrink refused at dtmin": negative and not held and r["dt_before"] * m["dtshrink"] < dtmin and r["dt"] == r["dt_before"],
                "P <= 0 inside the initial delay leaves dt alone": negative and held and r["iter"] > 1 and r["dt"] == r["dt_before"],
                "P <= 0 after iteration 1 with halfstepback off": negative and r["iter"] > 1 and not m["halfstepback"],
                "dtv < dt": r["dtv"] < r["dt"],
                "delaystep 0": m["delaystep"] == 0,
                spec["style"]: True,
            }
            for k, v in hit.items():
                if v:
                    seen.setdefault(k, set()).add(spec["id"])
    print({k: len(v) for k, v in seen.items()}, f"farthest atom {far:.2f} A")
    for corner in ("dt == dtmax with tmax < 10", "a shrink refused at dtmin", "P <= 0 inside the initial delay leaves dt alone",
                   "P <= 0 after iteration 1 with halfstepback off", "dtv < dt", "delaystep 0", "rebomos", "aeam"):
        assert corner in seen, f"no fire case of {nets.SUITE['fire']} reaches '{corner}'"


def test_heat_cases_run_clean_and_the_limits_are_the_references(oracle):
    """Needs the oracle, no GPU.  Every `heat` case of the suite runs through the reference without a HeatError and with its
    lowest escale above 0.5, reaches what its draw promises (a drifting source with vsub != 0, application counts that are
    the numbers of due steps), and the limits the device is held to are the reference's own: against the plain run
      (i)  every source's atoms summed in a random order stays 100 times inside every limit, and
      (ii) an error of +-1e-9 eV/A (uniform) on every force component at every step stays within a quarter of the position, velocity and scale
           limits (the state words vcm and ke are bounded from (i) alone)."""
    worst = {"i": dict.fromkeys(nets.HEAT_LIMITS, 0.0), "ii": dict.fromkeys(nets.HEAT_LIMITS, 0.0)}
    for spec in SPECS["heat"]:
        s, v0, by_tag, g, groups, flux, safe = nets._heat_system(spec)
        assert not any((a & b).any() for i, a in enumerate(groups) for b in groups[:i]) and not any((l & ~g).any() for l in groups)
        if spec["shapes"][-1]["kind"] == "rest":
            assert np.array_equal(np.logical_or.reduce(groups), g)
        ref, lowest = nets.heat_reference(spec)
        assert lowest > 0.5, (spec["id"], lowest)
        last = ref[spec["nsteps"]][3]
        for k, q in enumerate(last):
            assert q["applied"] == sum((nets.heat_due(spec, n) >> k) & 1 for n in range(1, spec["nsteps"] + 1)), (spec["id"], k)
        q = last[spec["drifting"]]
        assert q["applied"] == 0 or spec["c"][spec["drifting"]] == 0.0 or np.all((q["scale"] - 1.0) * q["vcm"] != 0.0), spec["id"]
        for name, other in (("i", nets.heat_reference(spec, permuted=True)[0]), ("ii", nets.heat_reference(spec, dforce=1e-9)[0])):
            w = nets.heat_worst(spec, s, g, ref, other)
            for k in worst[name]:
                worst[name][k] = max(worst[name][k], w[k])
            print(spec["id"], name, {k: f"{v:.1e}" for k, v in w.items()})
    print("worst of (i):", {k: f"{v:.2e}" for k, v in worst["i"].items()})
    print("worst of (ii):", {k: f"{v:.2e}" for k, v in worst["ii"].items()})
    # nets.HEAT_LIMITS were set from these two lines of output for THIS seed and case count (4 x (ii), 100 x (i)), so some
    # margins below are a few per cent by construction: after a change of the seed, the case count, the draw or the oracle's
    # rounding, set the limits again from what is printed above (see the note at nets.HEAT_LIMITS)
    for k, lim in nets.HEAT_LIMITS.items():
        assert worst["i"][k] < 0.01 * lim, (k, worst["i"][k], lim)
    for k in ("dx", "dv", "dscale"):
        assert worst["ii"][k] < 0.25 * nets.HEAT_LIMITS[k], (k, worst["ii"][k])


_PF = {}


def _postforce(spec):
    """(the case as nets._pf_system fits it, its plain reference, what that run showed), once per case"""
    if spec["id"] not in _PF:
        P = nets._pf_system(spec)
        _PF[spec["id"]] = (P,) + nets.postforce_reference(spec, P)
    return _PF[spec["id"]]


def postforce_conditions(specs):
    """the reference alone over `postforce` cases: asserts what every case promises and returns what the cases reach together"""
    reach = dict(wraps=set(), sheared_wraps=set(), rzero=False, zflag_sheared=False, emptied=False, decided=False)
    for spec in specs:
        P, ref, seen = _postforce(spec)
        last = ref[spec["nsteps"]]
        assert all(np.isfinite(w[0]).all() and np.isfinite(w[2]).all() for w in ref.values()), spec["id"]
        print(spec["id"], {k: ([round(a, 3) for a in v] if isinstance(v, list) and v and isinstance(v[0], float) else v) for k, v in seen.items()})
        for k, q in enumerate(P["inds"]):
            if q["k"] > 0.0:
                assert seen["contacts"][k] >= 2, (spec["id"], k, seen["contacts"])
                assert seen["deepest"][k] < 0.8, (spec["id"], k, seen["deepest"])
                assert seen["fmax"][k] >= 0.05, (spec["id"], k, seen["fmax"])
            if q["shape"] == "plane":   # clear of the faces by skin + 1.5 A at every step: the remap never touches its atoms
                assert seen["face"][k] >= spec["skin"] + nets.PF_FACE, (spec["id"], k, seen["face"])
                assert q["bit"] != 0
            else:
                reach["wraps"] |= seen["wraps"][k]
                if spec["tilt"]:
                    reach["sheared_wraps"] |= seen["wraps"][k]
            if q["shape"] == "cylinder":
                assert q["vel"][q["dim"]] == 0.0
        for k, (q, d) in enumerate(zip(P["springs"], spec["springs"])):
            if d["moving"] and q["k"] > 0.0:
                assert seen["sfmax"][k] >= 0.05, (spec["id"], k, seen["sfmax"])
            if d["r0"] == "above":
                assert ref[0][1][k]["dr"] < 0.0 and (q["k"] == 0.0 or ref[0][1][k]["ftotal"][3] < 0.0), (spec["id"], k)
        reach["rzero"] = reach["rzero"] or seen["rzero"]
        if spec["tilt"] and spec["springs"] and seen["zflag"]:
            reach["zflag_sheared"] = True
        if spec["newmask"] is not None:
            at, e = spec["newmask"]
            assert ref[at][1][e]["atoms"] > 0 and last[1][e]["atoms"] == 0 and last[1][e]["mass"] == 0.0 and not last[1][e]["ftotal"].any()
            reach["emptied"] = True
        if spec["free"] is not None:    # the free dimension decides: with the wrap taken there as well the energy is another
            assert spec["nsteps"] == 0 and list(ref) == [0]
            other = nets.postforce_reference(spec, P, periodic=(True, True, True))[0]
            assert abs(other[0][4][0]["energy"] - ref[0][4][0]["energy"]) > 1e-6, (spec["id"], other[0][4][0]["energy"], ref[0][4][0]["energy"])
            reach["decided"] = True
    return reach


def test_postforce_cases_meet_their_own_conditions(oracle):
    """Needs the oracle, no GPU.  Every `postforce` case of the suite runs clean through the reference (no stale list, finite
    throughout) and shows what its fit promises: every indenter with K > 0 touches at least 2 atoms at some read, never
    reaches deeper than 0.8 A into an atom it pushes (the atom of the r == 0 case feels no force and is left out) and puts at
    least 0.05 eV/A on one; every plane's atoms stay skin + 1.5 A clear of the faces whose remap would change their
    coordinate along dim; every moving spring with K > 0 reaches |F| = 0.05 eV/A; a rest length above the distance pushes; a
    case with a free dimension has another energy once the wrap is taken there as well.  Over the suite: in each of x, y and z
    an atom in contact takes the wrap, in a sheared box in z and in y; an r == 0 contact is counted; in a sheared cell an
    atom of a spring's group changes its z image flag in mid-run; a spring loses its group to a new mask."""
    reach = postforce_conditions(SPECS["postforce"])
    print(reach)
    assert reach["wraps"] == {0, 1, 2} and reach["sheared_wraps"] >= {1, 2}, reach
    assert reach["rzero"] and reach["zflag_sheared"] and reach["emptied"] and reach["decided"], reach


def test_postforce_limits_are_the_references(oracle):
    """Needs the oracle, no GPU.  The limits of the `postforce` net are the reference's own: over the suite's cases, against the
    plain run,
      (i)  every stage's atoms summed in a random order stays 100 times inside every limit, and
      (ii) an error of +-1e-9 eV/A (uniform) on every force component at every step stays within a quarter of every limit;
    a limit that differs from the project's bound for the quantity (nets.PF_START) is the larger of 100 x (i) and 4 x (ii),
    rounded up in the second digit."""
    worst = {"i": dict.fromkeys(nets.PF_START, 0.0), "ii": dict.fromkeys(nets.PF_START, 0.0)}
    for spec in SPECS["postforce"]:
        P, ref, _ = _postforce(spec)
        for name, other in (("i", nets.postforce_reference(spec, P, permuted=True)[0]), ("ii", nets.postforce_reference(spec, P, dforce=1e-9)[0])):
            w = nets.postforce_worst(spec, P, ref, other)
            assert w["exact"] == 0, (spec["id"], name)
            for k in worst[name]:
                worst[name][k] = max(worst[name][k], w[k])
            print(spec["id"], name, {k: f"{w[k]:.1e}" for k in worst[name]})
    print("worst of (i):", {k: f"{v:.2e}" for k, v in worst["i"].items()})
    print("worst of (ii):", {k: f"{v:.2e}" for k, v in worst["ii"].items()})
    # after a change of the seed, the case count, the draw or the oracle's rounding, set nets.PF_LIMITS again from what is
    # printed above -- never from what the device gives
    for k, lim in nets.PF_LIMITS.items():
        assert worst["i"][k] < 0.01 * lim, (k, worst["i"][k], lim)
        assert worst["ii"][k] < 0.25 * lim, (k, worst["ii"][k], lim)
        need = max(100.0 * worst["i"][k], 4.0 * worst["ii"][k])
        assert lim == nets.PF_START[k] or lim < 1.2 * need, (k, lim, need, "a limit wider than the experiments ask for")


def test_measure_grid_restatement():
    """nets.measure_bin_grid against bin_grid of csrc/measure_bin.hip worked by hand: a 43.27 A cube (the 6-cell alloy's box,
    7.5 + 2 A further each way) with 3 700 atoms has the cap 4 x 3700 + 4096 = 18 896; cells of 1.5 A are 28^3 = 21 952, above
    it, and cells of 1.5 x 1.26 = 1.89 A are 22^3 = 10 648; cells of 1.6 A are 27^3 = 19 683, still above; cells of 3.25 A
    (the cutoff at its limit) are 13^3"""
    lens = [4.045 * 6 + 2 * 9.5] * 3
    assert nets.measure_bin_grid(lens, 3.0, 3700) == ([22, 22, 22], 1)
    assert nets.measure_bin_grid(lens, 3.2, 3700) == ([21, 21, 21], 1)
    assert nets.measure_bin_grid(lens, 6.5, 3700) == ([13, 13, 13], 0)
    assert nets.measure_bin_grid([5000.0, 1.0, 1.0], 2.0, 10) == ([1024, 1, 1], 0)
    s = nets.S.fcc_cell(4.045, 6)
    assert np.allclose(nets.measure_domain_lens(s.box, 7.5), lens)
    # 864 atoms, 1 + 2 x 7.5 / 24.27 = 1.618 per periodic dimension, 5 % more
    assert nets.measure_nall_bound(s.box, 864, 7.5) == int(np.ceil(1.05 * 864 * (1 + 15 / 24.27) ** 3))
    assert nets.measure_nall_bound(s.box, 864, 7.5, (0, 0, 1)) == int(np.ceil(1.05 * 864 * (1 + 15 / 24.27) ** 2))


def test_measure_cases_meet_their_own_conditions():
    """No GPU, no oracle.  On the start positions of every `measure` case of the suite the references meet the conditions
    the case sets itself: at most 2 edge events (edge pairs, edge angles, neighbours at a shell radius), no centre with
    more than 100 neighbours inside the largest outer radius (the device's list holds 128; the margin is for thermal
    motion), and -- unless the case is about a tiny group or one type left out -- at least 3e4 rdf entries and 3e4 angles
    (three times the floor of a read, for what thermal motion takes out of a first shell); the draw's own counts of entries
    and angles are the references'."""
    for spec in SPECS["measure"]:
        s = nets._cell_start(spec)
        member = nets.group_member(spec, s)
        rref, aref = nets.measure_references(spec, s.x, s.type, s.box.h, member)
        entries, angles = int(rref["hist"].sum()), int(aref["hist"].sum())
        print(spec["id"], f"{entries} entries, {angles} angles, at most {aref['max_neighbours']} neighbours, edge events "
              f"{rref['n_edge']} + {aref['n_edge']} + {aref['n_shell_edge']}")
        assert rref["n_edge"] + aref["n_edge"] + aref["n_shell_edge"] <= 2, spec["id"]
        assert aref["max_neighbours"] <= nets.MSR_NEIGH, (spec["id"], aref["max_neighbours"])
        limit = nets.MSR_LIMIT[spec["style"]]
        assert all(0.0 <= t[k] < t[k + 1] <= limit for t in spec["triples"] for k in (6, 8)), spec["id"]
        assert spec["cutoff"] is None or nets.MSR_FIRST[spec["style"]] < spec["cutoff"] < limit
        pairs = nets._msr_pairs(s, spec, limit)
        assert (entries, angles) == nets.measure_start_counts(spec, s, member, pairs), spec["id"]
        if spec["group"]["kind"] == "tiny":
            assert member.sum() in (2, 3)
        elif spec["group"]["kind"] != "one type out":
            assert entries >= nets.MSR_FLOOR_START and angles >= nets.MSR_FLOOR_START, (spec["id"], entries, angles)


def test_peratom_cases_meet_their_own_conditions():
    """No GPU, no oracle.  On the start state of every `peratom` case of the suite the reference alone meets the conditions the
    case sets itself: at most 2 atoms within 1e-9 of a bin edge in either grid (expected n x sum(nbin) x 2e-9, below 1e-2),
    the premise of the image check (1.5 x the speed cap x dt x the steps between two reads stays below half the smallest
    perpendicular width), a step between two list builds under the rule of _cell_velocities where the drift is fast, the
    group the case names (nobody: no member; a few: 1 - 3), zero velocities at 0 K, and the reference passes its own check"""
    import profileref
    for spec in SPECS["peratom"]:
        s = nets._cell_start(spec)
        v0, safe = nets._cell_velocities(spec, s)
        member = nets.peratom_member(spec, s)
        kind = spec["group"]["kind"]
        assert (member is None) == (kind == "none")
        if kind == "nobody":
            assert not member.any()
        elif kind == "few":
            assert member.sum() == spec["group"]["count"] in (1, 2, 3)
        elif kind != "none":
            assert 0 < member.sum() < s.n
        if spec["temp"] == 0:
            assert not v0.any() and not any(spec["drift"])
        if spec["fast_on"]:
            assert nets.PA_FAST in np.abs(spec["drift"]) and int(0.3 * nets.MSR_SKIN[spec["style"]] / (spec["vcap"] * nets.PA_DT)) >= 1
        reads = sorted({0, spec["between"], spec["nsteps"]})
        assert 0 < spec["between"] < spec["nsteps"] and spec["nsteps"] >= 5
        assert 1.5 * spec["vcap"] * nets.PA_DT * max(np.diff(reads)) < 0.98 * nets.peratom_half_width(s.box)
        per = tuple(bool(p) for p in nets._cell_periodic(spec))
        lam = s.box.x2lamda(s.x)
        for dims, nbins in spec["grids"]:
            assert s.n * sum(nbins) * 2e-9 < 1e-2, spec["id"]
            ref = profileref.table(lam, per, dims, nbins, s.mass[s.type], v0, member=member, natoms_total=s.n)
            edge = profileref.edges(lam, per, dims, nbins, member)
            assert edge["n_edge"] <= 2, (spec["id"], edge["n_edge"])
            profileref.check_sums_with_edges(ref["count"], ref["sums"], ref["exponents"], ref, edge)
            assert ref["count"].sum() == (s.n if member is None else member.sum())


def structure_conditions(specs):
    """the references alone on the start positions of `structure` cases: asserts what every case promises and returns what the
    cases reach together: the cna patterns, the neighbour counts of the centres, the centres with 12 or 14 neighbours that are
    `other`"""
    import cnaref
    seen = dict(patterns=set(), neighbours=set(), other_at_12_or_14=0)
    for spec in specs:
        s = nets._cell_start(spec)
        member = nets.peratom_member(spec, s)
        sel = np.ones(s.n, dtype=bool) if member is None else member
        kind, limit = spec["group"]["kind"], nets.MSR_LIMIT[spec["style"]]
        assert (member is None) == (kind == "none")
        if kind == "nobody":
            assert not member.any()
        elif kind == "few":
            assert member.sum() == spec["group"]["count"] in (1, 2, 3)
        pairs = nets._msr_pairs(s, spec, limit)
        exempt = kind in ("few", "nobody") or spec["cell"] == "icosahedron"
        for p in nets.structure_sets(spec):
            cref, zref, aref, ccut = nets.structure_references(spec, p, s.x, s.type, s.box.h, member)
            largest = max(p["coord_cutoff"], ccut, p["cna_cutoff"])
            assert largest <= limit and min(p["coord_cutoff"], ccut, p["cna_cutoff"]) > 0.0, spec["id"]
            assert (p["centro_cutoff"] is None) == (ccut == limit)
            most = int(np.bincount(pairs[0][pairs[2] < largest], minlength=s.n).max())
            edges = (cref["n_edge"], int(zref["ambiguous"].sum()), int(aref["ambiguous"].sum()))
            full = int((sel & (zref["inside"] >= p["nnn"])).sum())
            some = int((sel & (cref["count_sure"].sum(axis=1) > 0)).sum())
            print(spec["id"], f"at most {most} inside {largest:.3f}, edge events {edges}, {full} centres with N = {p['nnn']} inside {ccut:.3f}, "
                  f"{some} with a coordination number, cna {cnaref.histogram(aref['pattern']).tolist()}")
            assert most <= nets.MSR_NEIGH, (spec["id"], most)
            assert max(edges) <= 2, (spec["id"], edges)
            assert 2 <= p["nnn"] <= 64 and 1 <= len(p["cols"]) <= 32
            assert (full, some) == nets.structure_start_counts(spec, p, s, member, pairs) or cref["n_edge"] or zref["ambiguous"].any(), spec["id"]
            if not exempt:
                assert full >= nets.STR_FLOOR and some >= nets.STR_FLOOR, (spec["id"], full, some)
            seen["patterns"] |= set(aref["pattern"][sel].tolist())
            seen["neighbours"] |= set(aref["neighbours"][sel].tolist())
            seen["other_at_12_or_14"] += int((sel & np.isin(aref["neighbours"], (12, 14)) & (aref["pattern"] == cnaref.OTHER)).sum())
    return seen


def test_structure_cases_meet_their_own_conditions():
    """No GPU, no oracle.  On the start positions of every `structure` case of the suite, for each of its parameter sets, the
    references alone meet the conditions the case sets itself: no centre has more than 100 atoms inside the largest cutoff
    (the short list holds 128; the margin is for thermal motion); at most 2 edge pairs (coord) and 2 ambiguous atoms (centro,
    cna); every cutoff at most the ghost shell's limit; unless the case is about a group of 0 - 3 atoms or the 13-atom
    icosahedron, at least 100 centres have N atoms inside centro's cutoff and at least 100 a non-zero coordination number in
    some column, and the draw's own counts of both are the references'.  Over the whole suite the reference's cna patterns
    are fcc, hcp, bcc, icosahedral and other; centres with 13, 15, 16 and 17 neighbours occur (the edges of the list of 16
    and of the n == 12 || n == 14 branch), and centres with 12 or 14 neighbours that are `other` all the same."""
    import cnaref
    seen = structure_conditions(SPECS["structure"])
    print(seen)
    assert seen["patterns"] >= {cnaref.FCC, cnaref.HCP, cnaref.BCC, cnaref.ICO, cnaref.OTHER}
    assert seen["neighbours"] >= {13, 15, 16, 17} and seen["other_at_12_or_14"] >= 1
