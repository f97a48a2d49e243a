"""CPU: groups at the plugin boundary and in the mini-host.  The mini-host's `group` forms, `velocity ID set` and
`write_dump` on host-only inputs; the refusals of the device fixes and of `minimize/mdp ... group` that need no device
-- an unknown group ID, an empty group, a Langevin group with atoms the integrator does not move -- each with a message
naming the problem."""
import os

import pytest

from test_plugin_boundary import HEAD, _run

GROUPS = HEAD + """region low block 0 2 0 2 0 0.6
region band block 0 2 0.9 1.6 0 2
group bottom region low
group mobile subtract all bottom
group inband region band
group strip intersect inband mobile
group silicon type 2
group few id 1:3 7 30:32
"""


def test_group_forms_count_their_atoms():
    rc, out, err = _run(GROUPS)
    assert rc == 0, err
    # 2 x 2 x 2 fcc cells, 32 atoms in layers of 8 at 0, a/2, a, 3a/2: `low` holds the z layers at 0 and a/2, `band` the y
    # layers at a and 3a/2
    for line in ("16 atoms in group bottom", "16 atoms in group mobile", "16 atoms in group inband", "8 atoms in group strip",
                 "0 atoms in group silicon", "7 atoms in group few"):
        assert line in out, (line, out)


@pytest.mark.parametrize("cmd,msg", [
    ("group all type 1", "Group all cannot be redefined"),
    ("group g region nosuch", "Group region nosuch does not exist"),
    ("group g subtract all nosuch", "Group ID nosuch does not exist"),
    ("group g molecule 1", "minilmp supports `group ID region R`"),
    ("group g id 1:x", "neither a number nor a range"),
    ("velocity nosuch set 0 0 0", "Could not find velocity group ID nosuch"),
    ("write_dump nosuch custom x.dump id x y z vx vy vz", "Could not find dump group ID nosuch"),
    ("write_dump all custom x.dump id type x y z", "minilmp supports `write_dump ID custom FILE id x y z vx vy vz` only"),
    ("fix 1 nosuch nve", "Could not find fix group ID nosuch"),
])
def test_mini_host_refusals(cmd, msg):
    rc, out, err = _run(GROUPS + cmd + "\n")
    assert rc == 1
    assert msg in err, err


def test_velocity_set_and_write_dump(tmp_path):
    """rows sorted by id, %.17g: the values read back are the doubles the host holds"""
    dump = tmp_path / "bottom.dump"
    rc, out, err = _run(GROUPS + "velocity all create 300.0 4711\nvelocity bottom set 0.1 -0.25 1.0e-3\n"
                        f"write_dump bottom custom {dump} id x y z vx vy vz\nwrite_dump all custom {tmp_path / 'all.dump'} id x y z vx vy vz\n")
    assert rc == 0, err
    lines = dump.read_text().splitlines()
    assert lines[:5] == ["ITEM: TIMESTEP", "0", "ITEM: NUMBER OF ATOMS", "16", "ITEM: ATOMS id x y z vx vy vz"]
    rows = [l.split() for l in lines[5:]]
    ids = [int(r[0]) for r in rows]
    assert ids == sorted(ids) and len(ids) == 16
    for r in rows:
        assert [float(v) for v in r[4:]] == [0.1, -0.25, 1.0e-3]
        assert float(r[3]) in (0.0, 2.0225)                    # the two layers of the region
    every = (tmp_path / "all.dump").read_text().splitlines()[5:]
    assert len(every) == 32
    moving = [l.split() for l in every if int(l.split()[0]) not in ids]
    assert all(float(r[4]) != 0.1 for r in moving)             # the others kept the velocities `create` drew
    assert any(len(r[4]) >= 17 for r in moving)                # %.17g: every digit of a drawn velocity


NVE = "plugin load rebomosplugin.so\n"
LGV = NVE + "plugin load langevinmdpplugin.so\n"


@pytest.mark.parametrize("head,cmds,msg", [
    (NVE, "fix 1 nosuch nve/mdp", "Fix nve/mdp requires group all or a group defined by the group command: could not find fix group ID nosuch"),
    ("plugin load nvtmdpplugin.so\n", "fix 1 nosuch nvt/mdp temp 300 300 0.1",
     "Fix nvt/mdp requires group all or a group defined by the group command: could not find fix group ID nosuch"),
    (LGV, "fix 2 nosuch langevin/mdp 300 300 0.1 48271",
     "Fix langevin/mdp requires group all or a group defined by the group command: could not find fix group ID nosuch"),
    (NVE, "fix 1 silicon nve/mdp", "Fix nve/mdp: group silicon is empty"),
    ("plugin load nvtmdpplugin.so\n", "fix 1 silicon nvt/mdp temp 300 300 0.1", "Fix nvt/mdp: group silicon is empty"),
    (LGV, "fix 2 silicon langevin/mdp 300 300 0.1 48271", "Fix langevin/mdp: group silicon is empty"),
    (LGV, "fix 1 mobile nve/mdp\nfix 2 inband langevin/mdp 300 300 0.1 48271",
     "Fix langevin/mdp: group inband has 8 atoms outside group mobile of fix 1 (nve/mdp)"),
    (LGV, "fix 1 mobile nve/mdp\nfix 2 all langevin/mdp 300 300 0.1 48271",
     "Fix langevin/mdp: group all has 16 atoms outside group mobile of fix 1 (nve/mdp)"),
    ("plugin load minimizemdpplugin.so\n", "minimize/mdp 0.0 1.0e-6 100 1000 group nosuch", "minimize/mdp: could not find group ID nosuch"),
    ("plugin load minimizemdpplugin.so\n", "minimize/mdp 0.0 1.0e-6 100 1000 group silicon", "minimize/mdp: group silicon is empty"),
    ("plugin load minimizemdpplugin.so\n", "minimize/mdp 0.0 1.0e-6 100 1000 group", "minimize/mdp: group needs a group ID"),
])
def test_plugin_refusals_before_a_device_is_touched(head, cmds, msg):
    rc, out, err = _run(head + GROUPS + cmds + "\n")
    assert rc == 1
    assert msg in err, err


def test_defined_groups_are_accepted_by_every_device_style():
    rc, out, err = _run(LGV + "plugin load nvtmdpplugin.so\n" + GROUPS +
                        "fix 1 mobile nve/mdp\nfix 2 strip langevin/mdp 300 300 0.1 48271 zero yes tally yes\nunfix 2\n"
                        "fix 1 mobile nvt/mdp temp 300 300 0.1\n")
    assert rc == 0, err
