"""The decode step's layer plan (gpt2_decode_layer_plan, paged_infer.c
dec_plan): what every request 0..7 of gpt2_decode_set_layer_kernel becomes for
a shape, KV dtype, weight dtype and CU count.  The function is pure, so the
table holds without a GPU (num_cus = 256, the MI355X's).

Each entry is (form, chain, first); FIVE rows check form 0 and first 0 only.
attn_launch is 1 exactly for forms 2..5 and splits is 1 in every row of the
product build (only form 1, the full persistent layer of A/B builds, runs
attention ranges inside the layer launch).  The rows restate what the routing
section of tests/test_gpu_kv_fp8.py, tests/test_gpu_configs.py,
tests/test_gpu_layer.py and tests/test_gpu_pipe.py assert on the GPU.

An A/B library (-DHPA_AB, HPA_LIB=...) answers differently for requests 2, 4
and 7 only; those rows carry both answers.

One GPU test ties the function to the engine: for every request, what the
engine reports (Model.layer_form) is the plan's form at the device's CU count."""
import numpy as np
import pytest

import pagedattn as pa

F32, BF16, FP8 = pa.HPA_F32, pa.HPA_BF16, pa.HPA_FP8
FIVE = (0, None, 0)
MAX_CTX = 1024


def _plan(request, B, C, NH, kv=F32, w_bf16=False, num_cus=256, pick_B=None, max_ctx=MAX_CTX):
    return pa.layer_plan(request, B, C, NH, max_ctx, kv, w_bf16, num_cus, pick_B)


def _check(p, expect, what):
    form, chain, first = expect
    assert p["form"] == form, (what, p)
    assert p["first"] == first, (what, p)
    if chain is not None:
        assert p["chain"] == chain, (what, p)
    assert p["attn_launch"] == (1 if 2 <= form <= 5 else 0), (what, p)
    if form != 1:
        assert p["splits"] == 1, (what, p)


def _ab():
    return bool(pa.lib().hpa_build_flags() & 1)


def _rows():
    """(what, kwargs of _plan without the request, {request: product answer})"""
    rows = []
    for B in (1, 16, 17, 64):
        rows.append((f"124M fp32 B={B}", dict(B=B, C=768, NH=12),
                     {1: (3, 6, 1), 5: (3, 6, 1), 7: (3, 6, 1), 6: (3, 8, 1), 3: (2, 1, 0), 0: FIVE, 2: FIVE, 4: FIVE}))
    rows.append(("124M fp32 B=65", dict(B=65, C=768, NH=12), {r: FIVE for r in range(8)}))
    rows.append(("124M bf16 KV B=64", dict(B=64, C=768, NH=12, kv=BF16),
                 {1: (3, 6, 1), 5: (3, 6, 1), 7: (3, 6, 1), 6: (3, 8, 1), 3: (2, 1, 0), 0: FIVE, 2: FIVE, 4: FIVE}))
    rows.append(("C=1024 B=4", dict(B=4, C=1024, NH=16),
                 {1: (3, 8, 0), 6: (3, 8, 0), 0: FIVE, 2: FIVE, 3: FIVE, 4: FIVE, 5: FIVE, 7: FIVE}))
    rows.append(("XL B=64", dict(B=64, C=1600, NH=25),
                 {1: (3, 8, 0), 6: (3, 8, 0), 0: FIVE, 2: FIVE, 3: FIVE, 4: FIVE, 5: FIVE, 7: FIVE}))
    rows.append(("C=128 B=4", dict(B=4, C=128, NH=2),
                 {1: (2, 1, 0), 3: (2, 1, 0), 4: (2, 1, 0), 5: (2, 1, 0), 7: (2, 1, 0), 0: FIVE, 2: FIVE, 6: FIVE}))
    rows.append(("124M fp8 KV B=20", dict(B=20, C=768, NH=12, kv=FP8),
                 {1: (3, 6, 1), 5: (3, 6, 1), 0: FIVE, 2: FIVE, 3: FIVE, 4: FIVE, 6: FIVE, 7: FIVE}))
    rows.append(("C=1280 fp8 KV", dict(B=4, C=1280, NH=20, kv=FP8), {r: FIVE for r in range(8)}))
    rows.append(("C=128 fp8 KV", dict(B=4, C=128, NH=2, kv=FP8), {r: FIVE for r in range(8)}))
    rows.append(("124M fp8 KV bf16 weights", dict(B=20, C=768, NH=12, kv=FP8, w_bf16=True),
                 {r: FIVE for r in range(8)}))
    for kv in (F32, BF16):
        for B in (4, 64, 256):
            rows.append((f"124M bf16 weights kv={kv} B={B}", dict(B=B, C=768, NH=12, kv=kv, w_bf16=True),
                         {**{r: (4, None, 2) for r in range(1, 8)}, 0: FIVE}))
    # the bf16 chain: C = 768 and <= 256 rows only
    rows.append(("124M bf16 weights B=257", dict(B=257, C=768, NH=12, w_bf16=True), {r: FIVE for r in range(8)}))
    rows.append(("C=1024 bf16 weights", dict(B=4, C=1024, NH=16, w_bf16=True), {r: FIVE for r in range(8)}))
    # no device: nothing is eligible
    for kw in (dict(B=4, C=768, NH=12), dict(B=4, C=128, NH=2), dict(B=4, C=768, NH=12, w_bf16=True)):
        rows.append((f"no CUs {kw}", dict(num_cus=0, **kw), {r: FIVE for r in range(8)}))
    # a CU count that is no multiple of 8 (the 4-wave chain's grid) or too small for a unit per workgroup
    rows.append(("C=128 on 100 CUs", dict(B=4, C=128, NH=2, num_cus=100), {1: FIVE, 3: FIVE}))
    rows.append(("124M B=64 on 128 CUs", dict(B=64, C=768, NH=12, num_cus=128), {1: FIVE, 5: FIVE, 3: FIVE}))
    rows.append(("124M B=16 on 128 CUs", dict(B=16, C=768, NH=12, num_cus=128), {1: FIVE, 3: (2, 1, 0)}))
    rows.append(("124M B=32 on 192 CUs", dict(B=32, C=768, NH=12, num_cus=192), {1: (3, 6, 1), 3: (2, 1, 0)}))
    return rows


# requests 2, 4, 7 in an A/B library: the full layer (its splits by shape),
# the wide units of 1 + ceil(pick_B / 16), the pipelined halves at 17..64 rows
# of an fp32 pool
AB = {
    ("124M fp32 B=1", 2): (1, 0, 0), ("124M fp32 B=16", 2): (1, 0, 0), ("124M fp32 B=17", 2): (1, 0, 0),
    ("124M fp32 B=64", 2): (1, 0, 0), ("124M bf16 KV B=64", 2): (1, 0, 0), ("C=128 B=4", 2): (1, 0, 0),
    ("124M fp32 B=1", 4): (3, 2, 0), ("124M fp32 B=16", 4): (3, 2, 0), ("124M fp32 B=17", 4): (3, 3, 0),
    ("124M fp32 B=64", 4): (3, 5, 0), ("124M bf16 KV B=64", 4): (3, 5, 0),
    ("124M fp32 B=17", 7): (5, 6, 1), ("124M fp32 B=64", 7): (5, 6, 1),
}


def test_plan_table():
    ab = _ab()
    for what, kw, answers in _rows():
        for request, expect in answers.items():
            if ab:
                expect = AB.get((what, request), expect)
            _check(_plan(request, **kw), expect, (what, request))


def test_request_is_clamped():
    """as gpt2_decode_set_layer_kernel: below 0 is 0, above 7 is 7"""
    kw = dict(B=16, C=768, NH=12)
    assert _plan(-3, **kw) == _plan(0, **kw)
    assert _plan(99, **kw) == _plan(7, **kw)


def test_eligibility_on_own_batch_widths_on_global():
    """a shard of 8 rows told a global batch: eligibility is tested on its own
    8 rows, the 64-row limit of the persistent forms on the batch the picks
    follow"""
    _check(_plan(1, B=8, C=768, NH=12, pick_B=64), (3, 6, 1), "shard of 64")
    _check(_plan(1, B=8, C=768, NH=12, pick_B=65), FIVE, "picks follow 65 rows")
    _check(_plan(1, B=65, C=768, NH=12, pick_B=64), FIVE, "65 own rows")
    if _ab():  # the wide units' width follows the global batch
        _check(_plan(4, B=8, C=768, NH=12, pick_B=40), (3, 4, 0), "widths of 40 rows")


def test_full_layer_splits_follow_the_split_pick():
    """form 1 (A/B builds; five launches otherwise): the ranges inside the layer
    launch are hpa_decode_layer_pick_splits_cus of the pick batch"""
    L = pa.lib()
    for B in (1, 4, 16, 64):
        p = _plan(2, B=B, C=768, NH=12)
        if not _ab():
            _check(p, FIVE, B)
            continue
        assert p["form"] == 1 and p["chain"] == 0 and p["attn_launch"] == 0
        assert p["splits"] == L.hpa_decode_layer_pick_splits_cus(B, 12, MAX_CTX, 256)


def test_null_output_fails():
    assert pa.lib().gpt2_decode_layer_plan(1, 4, 4, 768, 12, 1024, 0, 0, 256, None) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("kv", [F32, FP8])
@pytest.mark.parametrize("C,NH", [(768, 12), (128, 2)])
def test_engine_reports_the_plans_form(hip, C, NH, kv):
    """2 layers, B = 4, page 16: after every set_layer_kernel(0..7) the engine's
    form is gpt2_decode_layer_plan's for the device's CU count; one step under
    the last request completes cleanly"""
    import synth
    cfgd = dict(maxT=128, V=512, L=2, NH=NH, C=C)
    B = 4
    num_cus = hip.device_info()[1]
    m = hip.Model(cfgd, params=synth.params(cfgd, seed=5))
    try:
        m.decode_init(B, 16, cfgd["maxT"], kv_dtype=kv)
        for request in range(8):
            m.set_layer_kernel(request)
            want = _plan(request, B, C, NH, kv, num_cus=num_cus, max_ctx=cfgd["maxT"])
            assert m.layer_form() == want["form"], (request, want)
        nxt = m.step(np.arange(B, dtype=np.int32))
        m.status()
        assert ((0 <= nxt) & (nxt < cfgd["V"])).all()
    finally:
        m.close()
