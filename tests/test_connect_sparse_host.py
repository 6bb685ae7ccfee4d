"""DeviceNetwork.connect_sparse checks its plan before it calls the library: entries that are not
(pre_id, post_id, ConnectionRule, WeightRule or None) raise TypeError, without a device."""
import ctypes

import pytest

from snn_amd import ConnectionRule, DeviceNetwork, WeightRule, _lib


class Recorder:
    """stands where the loaded library does: no call may reach it"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called for a plan that is not made of rules")


def bare():
    dn = DeviceNetwork.__new__(DeviceNetwork)          # (no handle: the constructor needs a device)
    dn._L, dn._h = Recorder(), _lib.H()
    return dn


@pytest.mark.parametrize("plan", [[(0, 1, "all_to_all", None)], [(0, 1, ConnectionRule.all_to_all(), 1.0)],
                                  [(0, 1, ConnectionRule.all_to_all())], [ConnectionRule.all_to_all()],
                                  [(0, 1, WeightRule.constant(1.0), ConnectionRule.all_to_all())],
                                  [(0, 1, ConnectionRule.chebyshev(1), None), (0, 1, lambda x, y: True, None)]])
def test_connect_sparse_rejects_what_is_not_a_rule(plan):
    with pytest.raises(TypeError):
        bare().connect_sparse(plan)


def test_the_record_has_the_layout_of_the_header():
    assert ctypes.sizeof(_lib.ConnectRecord) == 56
    assert [(_lib.ConnectRecord.__dict__[n].offset) for n, _ in _lib.ConnectRecord._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 36, 40, 48]
