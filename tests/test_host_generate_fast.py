"""tests/test_gpu_generate_fast.py on the CPU: the device tests' own bodies while the product's ops drive the host-compiled library
(tests/host_product.py), as tests/test_host_segment_suite.py does for the older segment tests; the 1024 x 1024 image is left to the device."""
import pytest
import torch

import test_gpu_generate_fast as GF
from host_product import product_on_host


@pytest.fixture(scope="module", autouse=True)
def host(tmp_path_factory):
    saved = (torch.Tensor.cuda, GF._gpu, torch.cuda.is_available)
    with product_on_host(str(tmp_path_factory.mktemp("host_generate_fast"))):
        torch.Tensor.cuda = lambda self, *a, **k: self
        GF._gpu = lambda: None
        torch.cuda.is_available = lambda: True                 # (nothing here touches a GPU)
        try:
            yield
        finally:
            torch.Tensor.cuda, GF._gpu, torch.cuda.is_available = saved


def test_patterns_are_what_they_claim():
    """The spiral and the comb are one component, the diagonal pair two, the checkerboard one per pixel (oracle only)."""
    for shape in [(37, 45), (64, 64), (513, 520)]:
        assert GF.case("spiral", shape)[1].max() == 1 and GF.case("comb", shape)[1].max() == 1
        assert GF.case("diagonal", shape)[1].max() == 2
        seg, ref, _ = GF.case("checkerboard", shape)
        assert ref.max() == (seg != 0).sum()
        assert (GF.case("spiral", shape)[0].sum(0) > 0).all()          # it reaches every column: every tile border is crossed


@pytest.mark.parametrize("shape", [(1, 1), (37, 45), (64, 64), (513, 520)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_level_labelling_is_the_oracles(shape):
    GF.test_two_level_labelling_is_the_oracles(shape)


@pytest.mark.parametrize("name", ["n1", "n63", "n64", "n65", "n130", "none_valid", "all_valid", "v64_of_130", "score_ties", "area_ties"])
def test_valid_limited_selection_is_the_operator_formulation_and_the_oracle(name):
    GF.test_valid_limited_selection_is_the_operator_formulation_and_the_oracle(name)
