"""CPU: every C-ABI call the Python host path makes - each field of each argument block, each allocation, each returned tensor's
shape / dtype / strides, each error message - equals the recording in tests/golden/host_calls.json (tests/host_calls.py makes it:
``python tests/host_calls.py --write``). The routes of flash_attn_interface.py may be rearranged under this test; what they hand to
the library may not move without the fixture showing exactly what moved."""
import pytest
import torch

import host_calls


@pytest.fixture(scope="module")
def golden():
    return host_calls.load_golden()


def test_case_list_and_fixture_agree(golden):
    assert sorted(golden) == sorted(host_calls.CASES)


@pytest.mark.parametrize("name", list(host_calls.CASES))
def test_host_calls_match_the_recording(name, golden):
    assert host_calls.run_case(name) == golden[name]


def test_combine_partials_refuses_an_output_type_the_library_has_no_code_for():
    """Not in the recording, which the parent of the refactor also had to match: there this call went to the library as bf16."""
    outs, lses = [torch.zeros(2, 40, 2, 64) for _ in range(2)], [torch.zeros(2, 2, 40) for _ in range(2)]
    calls = []
    with host_calls.stand_ins(calls=calls, allocs=[]):
        for dtype in (torch.float64, torch.float8_e4m3fn):
            with pytest.raises(RuntimeError, match="Output type must be FP32, FP16 or BF16"):
                host_calls.fai.combine_partials(outs, lses, out_dtype=dtype)
    assert calls == []
