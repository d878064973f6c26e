"""gpt2_decode_prefill_plan (pure, host only): request 1 answers 1 exactly
where hpa_paged_attention_prefill_packed applies, every other request 0; and
gpt2_decode_set_prefill_attention without an engine."""
import pytest

import pagedattn as pa

APPLIES = {pa.HPA_F32: (), pa.HPA_BF16: (8, 16, 32, 64), pa.HPA_FP8: (16, 32, 64)}


@pytest.mark.parametrize("request_", [0, 1, 2, -1])
@pytest.mark.parametrize("head_size", [64, 32, 128])
@pytest.mark.parametrize("kv_dtype", [pa.HPA_F32, pa.HPA_BF16, pa.HPA_FP8, 7])
def test_plan_table(kv_dtype, head_size, request_):
    for P in (1, 4, 8, 16, 24, 32, 64, 128):
        want = int(request_ == 1 and head_size == 64 and P in APPLIES.get(kv_dtype, ()))
        assert pa.prefill_plan(kv_dtype, P, head_size, request_) == want, P


@pytest.mark.parametrize("request_", [0, 1, 2])
def test_setter_without_an_engine_is_refused(request_):
    L = pa.lib()
    assert L.gpt2_decode_set_prefill_attention(None, request_) != 0
    model = L.gpt2_alloc()  # a model that gpt2_decode_init has not seen
    assert L.gpt2_decode_set_prefill_attention(model, request_) != 0
