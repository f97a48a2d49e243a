"""GPU: the randomised parity nets of tests/nets.py at the fixed seeds of nets.SUITE, one test item per case.  An item's id
names the net, the seed and the case index, so a failure reproduces with `python3 profiles/<net>_fuzz.py <index + 1>
<seed>` (the last line printed is the case).  tests/test_net_draws.py checks on the CPU that these seeds reach the
corners the nets exist for."""
import pytest

import nets

pytestmark = pytest.mark.gpu

CASES = [pytest.param(net, spec, id=f"{net}-seed{seed}-case{k}-{spec['id']}")
         for net, runs in nets.SUITE.items() for seed, n in runs for k, spec in enumerate(nets.cases(net, seed, n))]


@pytest.fixture(scope="module", autouse=True)
def _shared_context():
    yield
    nets.close_shared()      # (the context the REBO-MoS force cases share)


@pytest.mark.parametrize("net,spec", CASES)
def test_net_case(net, spec, monkeypatch):
    for k in nets.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in spec["env"].items():
        monkeypatch.setenv(k, v)
    err, lim = nets.NETS[net][1](spec)
    assert nets.passed(err, lim), nets.NETS[net][2](spec, err) + f"  limits {lim}"
