"""Host: the ``acc_slots`` argument of the packed state (tarl_hip.ops.FusedState) — its default, and the values it refuses
before anything is allocated. No GPU."""
import inspect

import pytest

from tarl_hip import ops


def test_default_bank_count_is_unchanged():
    assert ops.ACC_SLOTS == 32
    assert inspect.signature(ops.FusedState.__init__).parameters["acc_slots"].default == 32


@pytest.mark.parametrize("bad", [0, -1, -32, 4097, 2.0, "8", None, True])
def test_bad_bank_counts_are_rejected(bad):
    with pytest.raises(ValueError, match="acc_slots"):
        ops.FusedState(None, 4, 8, "cpu", 15, acc_slots=bad)
