"""gpt2_decode_dense_gemm_plan (pure, host only): 1 exactly for request 1 on
fp32 weights with K % 32 == 0; and the setter without an engine."""
import pytest

import pagedattn as pa


@pytest.mark.parametrize("request_", [0, 1, 2])
@pytest.mark.parametrize("K", [768, 784, 1600])
@pytest.mark.parametrize("w_dtype", ["HPA_F32", "HPA_BF16", "HPA_FP8", "HPA_FP4", "HPA_FP4A8"])
def test_plan_table(w_dtype, K, request_):
    want = int(request_ == 1 and w_dtype == "HPA_F32" and K % 32 == 0)  # 784 = 16 * 49
    assert pa.dense_gemm_plan(getattr(pa, w_dtype), K, request_) == want


def test_setter_without_an_engine_is_refused():
    L = pa.lib()
    assert L.gpt2_decode_set_dense_gemm(None, 1) != 0
    model = L.gpt2_alloc()  # a model that gpt2_decode_init has not seen
    assert L.gpt2_decode_set_dense_gemm(model, 1) != 0
