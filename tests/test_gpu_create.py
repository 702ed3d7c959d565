"""The requests bb_create refuses, on the GPU (`-m gpu`, MI355X): tests/_create_cases.py on the product library, the missing
device included.  Nothing is launched but the init kernels of the valid handle created after every refusal."""
import pytest

import _create_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cc.rows_for(gpu=True))
def test_refusal(hip_lib, name):
    cc.case_refusal(hip_lib, name)


def test_null_arguments(hip_lib):
    cc.case_null_arguments(hip_lib)


@pytest.mark.parametrize("kind", ["fitness", "multienv", "genotype", "replicate", "multienv_replicate"])
def test_base_request_is_valid(hip_lib, kind):
    cc.case_valid(hip_lib, kind)
