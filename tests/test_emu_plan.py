"""The launch plan of a handle, on the host emulation (g++ -DBB_EMU, no GPU): tests/_plan_cases.py against the emulation's column."""
import json
import os

import pytest

import _plan_cases as pc

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_emu.json")) as f:
    EXPECT = json.load(f)


@pytest.mark.parametrize("name", pc.rows_for(gpu=False))
def test_plan(emu_lib, monkeypatch, name):
    pc.case_plan(emu_lib, name, monkeypatch.setenv, EXPECT)
