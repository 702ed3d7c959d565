"""The requests bb_create refuses, on the host emulation (g++ -DBB_EMU, no GPU): tests/_create_cases.py."""
import pytest

import _create_cases as cc


@pytest.mark.parametrize("name", cc.rows_for(gpu=False))
def test_refusal(emu_lib, name):
    cc.case_refusal(emu_lib, name)


def test_null_arguments(emu_lib):
    cc.case_null_arguments(emu_lib)


@pytest.mark.parametrize("kind", ["fitness", "multienv", "genotype", "replicate", "multienv_replicate"])
def test_base_request_is_valid(emu_lib, kind):
    cc.case_valid(emu_lib, kind)
