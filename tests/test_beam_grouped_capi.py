"""Diverse beam search's surface on the CPU: the two names are declared, exported and wrapped; the setter's and the step's
refusals come before the device is touched, and the step fails loudly where there is no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from slimt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["slimt_hip_ctx_set_beam_groups", "slimt_hip_beam_step_grouped"]


def test_names_are_declared_exported_and_wrapped():
    header = open(os.path.join(ROOT, "include", "slimt_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS and getattr(capi.lib(), name).argtypes is not None, name
    assert callable(capi.beam_step_grouped) and callable(capi.Context.set_beam_groups)


@pytest.mark.parametrize("groups,penalty,message", [(2, float("nan"), "penalty"), (2, -1.0, "penalty"), (2, 1001.0, "penalty"),
                                                    (9, 0.5, "9 groups"), (-1, 0.5, "-1 groups"), (2, 0.5, "null argument")])
def test_the_setter_refuses_at_once(groups, penalty, message):
    L = capi.lib()
    assert L.slimt_hip_ctx_set_beam_groups(None, groups, ctypes.c_float(penalty), None) != 0
    assert message.encode() in L.slimt_hip_last_error()


def test_the_step_fails_loudly():
    lg, t, f = np.zeros((4, 5), np.float32), np.zeros(4, np.float32), np.ones(4, np.uint32)
    for groups, penalty, message in ((3, 0.0, "3 groups do not divide a beam of 4"), (0, 0.0, "0 groups"), (2, 1001.0, "penalty")):
        with pytest.raises(capi.SlimtHipError, match=message):
            capi.beam_step_grouped(lg, t, f, 4, groups, penalty)
    with pytest.raises(ValueError, match="beam_step_grouped"):
        capi.beam_step_grouped(lg, t[:3], f, 4, 2, 0.0)
    import torch
    if not torch.cuda.is_available():  # no device: an error, not a result
        with pytest.raises(capi.SlimtHipError):
            capi.beam_step_grouped(lg, t, f, 4, 2, 0.0)
