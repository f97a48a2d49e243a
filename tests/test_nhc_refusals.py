"""CPU: the thermostat of resident.DeviceDomain refuses several ranks before anything reaches a device, and the C-ABI
declares and exports the thermostat calls with the configuration layout the binding mirrors."""
import ctypes

import pytest

from lammps_plugins_amd.host import capi, resident


def test_device_domain_thermostat_refuses_several_ranks():
    d = object.__new__(resident.DeviceDomain)   # (no context: the refusal comes first)
    d.world = 2
    with pytest.raises(ValueError, match="one GPU only"):
        d.thermostat(300.0, 300.0, 0.1)


def test_nhc_exports_and_config_layout():
    L = capi.lib()
    for name in ("mdp_nhc_setup", "mdp_nhc_run", "mdp_nhc_state", "mdp_nhc_set_state", "mdp_nhc_off"):
        assert hasattr(L, name) and name in capi.EXPORTS
    assert ctypes.sizeof(capi.NhcConfig) == 3 * 8 + 2 * 4 + 4 * 8
    assert capi.NHC_STATE_LEN == 3 + 8 + 9 + 8
