"""gpt2_decode_prefill_plan under request 3 (pure, host only): 2 exactly where
hpa_paged_attention_prefill_split applies (fp32 pools), request 1's answer on
bf16 and fp8 pools, 0 everywhere else; and the setter without an engine."""
import pytest

import pagedattn as pa

SPLIT_PAGES = (8, 16, 32, 64)


@pytest.mark.parametrize("head_size", [64, 32, 128])
@pytest.mark.parametrize("kv_dtype", [pa.HPA_F32, pa.HPA_BF16, pa.HPA_FP8, 7])
def test_plan_table_request_3(kv_dtype, head_size):
    for P in (1, 4, 8, 16, 24, 32, 64, 128):
        if kv_dtype == pa.HPA_F32:
            want = 2 * int(head_size == 64 and P in SPLIT_PAGES)
        else:
            want = pa.prefill_plan(kv_dtype, P, head_size, 1)
        assert pa.prefill_plan(kv_dtype, P, head_size, 3) == want, P
    assert pa.prefill_plan(pa.HPA_FP8, 8, 64, 3) == 0 and pa.prefill_plan(pa.HPA_BF16, 8, 64, 3) == 1


def test_setter_without_an_engine_is_refused():
    L = pa.lib()
    assert L.gpt2_decode_set_prefill_attention(None, 3) != 0
    model = L.gpt2_alloc()  # a model that gpt2_decode_init has not seen
    assert L.gpt2_decode_set_prefill_attention(model, 3) != 0
