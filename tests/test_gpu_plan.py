"""The launch plan of a handle, on the GPU (`-m gpu`, MI355X): tests/_plan_cases.py on the product library against the column recorded
there.  Handles are created and their stats read; nothing is launched but the init kernels and, where a row switches the cross-GPU
leg on, the zero-step launch that warms the resident kernel."""
import json
import os

import pytest

import _plan_cases as pc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_gpu.json")) as f:
    EXPECT = json.load(f)


@pytest.mark.parametrize("name", pc.rows_for(gpu=True))
def test_plan(hip_lib, monkeypatch, name):
    pc.case_plan(hip_lib, name, monkeypatch.setenv, EXPECT)
