"""keep_reserve's promise (include/keep_hip.h): after reserve(tiles, prompts, seq) an encode of that size allocates nothing -- the arena
keep_workspace_bytes reports does not grow.  One case on each side of every branch of the sizing: graph-replayed calls (which stage their
inputs behind the workspace), one lane, two lanes, a ragged last lane, several rounds of max_tiles, chunks of max_prompts, and the
two-window state of split attention over more than 256 keys; in the default precision and in fp16, which carves no lo planes.
"""
import pytest
import torch

from keep_amd import KEEPModel, _lib
from keep_amd.config import small_shape
from keep_amd.synth import synth_state_dict, synth_tiles

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd():
    return synth_state_dict(small_shape(2, 2), seed=5)


def fresh_model(sd, precision, **options):
    m = KEEPModel(small_shape(2, 2), precision=precision)
    m.auto_calibrate = False
    m.trim_padding = False                 # encode_text at exactly the reserved length
    for k, v in options.items():
        m.set_option(k, v)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0").eval()


def workspace(m):
    return _lib.load().keep_workspace_bytes(m._handle)


# B = 1, 5: graph-replayed (985 <= 1024 token rows); 6: the first size that is not, one lane; 32: two lanes of 16; 33: a ragged second lane;
# 20 with max_tiles = 8: rounds of 8 + a remainder
@pytest.mark.parametrize("precision", ["comp", "fp16"])
@pytest.mark.parametrize("B,options", [(1, {}), (5, {}), (6, {}), (32, {}), (33, {}), (20, {"max_tiles": 8})],
                         ids=["1", "5", "6", "32", "33", "20_max_tiles_8"])
def test_reserved_image_encode_allocates_nothing(sd, precision, B, options):
    m = fresh_model(sd, precision, **options)
    assert workspace(m) == 0
    m.reserve(tiles=B)
    reserved = workspace(m)
    assert reserved > 0
    out = m.encode_image(synth_tiles(B, seed=3).cuda())
    torch.cuda.synchronize()
    assert out.shape == (B, 768) and bool(torch.isfinite(out).all())
    assert workspace(m) == reserved


# (1, 8); (64, 64): 4096 rows, the last graph-replayed size; (65, 64): chunks of max_prompts; (2, 300): split attention's two key windows
@pytest.mark.parametrize("precision", ["comp", "fp16"])
@pytest.mark.parametrize("P,T", [(1, 8), (64, 64), (65, 64), (2, 300)])
def test_reserved_text_encode_allocates_nothing(sd, precision, P, T):
    m = fresh_model(sd, precision)
    assert workspace(m) == 0
    m.reserve(prompts=P, seq=T)
    reserved = workspace(m)
    assert reserved > 0
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(4, 30522, (P, T), generator=g, dtype=torch.int64).cuda()
    out = m.encode_text({"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": torch.ones_like(ids)})
    torch.cuda.synchronize()
    assert out.shape == (P, 768) and bool(torch.isfinite(out).all())
    assert workspace(m) == reserved
