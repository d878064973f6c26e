"""Random engine call traces against a float64 model of every sequence.

One test per (profile, seed): one engine, one trace of tests/engine_model.py
(admissions, ragged calls, host- and device-fed steps, verify and tree-verify
passes, forks, releases, rewinds, reserve, one reset, and the graph / shared
attention / verify attention / attention splits toggles, interleaved), and
engine_model.check_op after EVERY op: positions, logits rows against the
float64 forward of each slot's token history, greedy ids, verify walks,
untouched slots bit for bit, K/V rows (prefixes bit for bit, written rows
against float64), free pages, the sharing pattern of a caller's BlockManager,
the shared-attention plan's invariants; releasing every slot at the end
returns every page.

Profiles (engine_model.PROFILES): f32-all (page 16, eager start), f32-shared-
graph (page 8, graph and shared attention on from the start, a caller's
manager of full capacity), bf16-pool (page 8; shared attention refused),
evict (B = 4, a caller's manager of 12 pages: the LRU policy pages sequences
out during steps, the model adopts gpt2_decode_evicted), chain6 (C = 768,
12 heads: the auto layer form is chain form 6, graph on).

Bars: 2e-4 (fp32 pools) and 5e-3 (bf16 pool) on |logit - float64 logit|, the
project's engine bars; tests/test_engine_model.py shows on the CPU that the
fp32 oracle sits bar / 16 or closer to the float64 decoder and what each class
of engine fault moves.  A failure names the check, the slot, the profile, the
seed and the op index i; make_trace(profile, seed, i + 1) reproduces it.

Eviction (the evict profile): the generator leaves evictions to the steps (a
ragged pass or a fork that pages out a slot of its own fails), so on the card
every eviction happens inside a step.  Held there: the op needed more fresh
pages than were free, and every page the evicted slot shared is still where
its other holders had it (their rows bit for bit, check 4).  "The evicted slot
held a page of its own" is always true in a step, where every slot gains one,
and is reached only by the CPU cases of tests/test_engine_model.py.

Measured on an MI355X, this file's own output (worst |engine - float64| / bar,
worst written K/V ratio / KV_RTOL, exempt near-tie rows / picks, evictions,
ops with a shared-attention unit live, seconds per test):

  profile            seed  ops  logit / bar  K/V / rtol  exempt    evict  units  s
  f32-all            1     80   0.002        0.005       1 / 174   -      -      0.3
  f32-all            2     80   0.001        0.004       0 / 163   -      -      0.3
  f32-all            3     80   0.001        0.005       0 / 158   -      -      0.3
  f32-shared-graph   1     80   0.001        0.004       0 / 167   -      14     0.4
  f32-shared-graph   2     80   0.001        0.005       0 / 159   -      11     0.3
  bf16-pool          1     60   0.002        0.000       3 / 152   -      -      0.3
  bf16-pool          2     60   0.009        0.009       4 / 147   -      -      0.3
  evict              1     60   0.001        0.004       0 / 151   4      -      0.2
  evict              2     60   0.002        0.004       0 / 135   11     -      0.2
  chain6             1     50   0.007        0.009       0 / 115   -      -      0.5
  chain6             2     50   0.007        0.008       0 / 101   -      -      0.4

The file's total is 4.1 s.  These are measurements: the bars stay the
project's.
"""
import time

import numpy as np
import pytest

import engine_model as em

pytestmark = pytest.mark.gpu

CASES = [(name, seed) for name, p in em.PROFILES.items() for seed in p["seeds"]]


def _manager(hip, profile):
    p = em.PROFILES[profile]
    if p["manager"] is None:
        return None
    per = p["cfg"]["maxT"] // p["P"]
    return hip.BlockManager(p["cfg"]["C"], max_prompts=p["B"], max_blocks=em.capacity(profile), block_size=p["P"],
                            max_blocks_per_prompt=per)


def _observe(hip, eng, m, bm, result=None):
    pos = eng.positions()
    nxt = np.zeros(m.B, np.int32)
    hip.check(hip.lib().hpa_memcpy(nxt.ctypes.data, eng.next_ptr(), nxt.nbytes), "next ids download")
    empty = np.zeros((0, m.cfg["C"]), np.float32)
    kv = [[eng.read_kv(l, b, int(pos[b])) if pos[b] else (empty, empty) for b in range(m.B)]
          for l in range(m.cfg["L"])]
    pages = refs = plan = None
    if bm is not None:
        pages = [bm.pages(b) for b in range(m.B)]
        refs = {pg: bm.refs(pg) for pl in pages for pg in pl}
        if eng.shared_attention():
            plan = eng.shared_plan()
    return em.Obs(pos, nxt, eng.logits(), kv, eng.free_pages(), pages, refs, plan, result)


def _run(eng, op):
    """one op on the engine; returns what the call itself reported"""
    k = op["kind"]
    if k in ("admit", "ragged"):
        return eng.prefill_ragged(op["seqs"])
    if k == "step_host":
        return eng.step(np.array(op["tokens"], np.int32))
    if k == "step_dev":
        return eng.step(None)
    if k == "verify":
        return eng.verify(op["drafts"])[:2]
    if k == "verify_tree":
        return eng.verify_tree(op["trees"])
    if k == "fork":
        eng.fork(op["src"], op["dst"], op["n"])
    elif k == "release":
        eng.release(op["slot"])
    elif k == "rewind":
        eng.set_positions(op["pos"])
    elif k == "reserve":
        eng.reserve(op["ctx"])
    elif k == "reset":
        eng.reset()
    elif k == "set_graph":
        eng.set_graph(op["on"])
    elif k == "set_shared":
        eng.set_shared_attention(op["on"], min_tiles=1, min_members=2, min_covered=2)
    elif k == "set_verify_attention":
        eng.set_verify_attention(op["request"])
    else:
        assert k == "set_attn_splits", k
        eng.set_attn_splits(op["splits"])
    return None


@pytest.mark.parametrize("profile,seed", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_trace(hip, profile, seed):
    t0 = time.time()
    p = em.PROFILES[profile]
    trace = em.make_trace(profile, seed)
    m = trace.model
    bm = _manager(hip, profile)
    eng = hip.Model(m.cfg, params=m.params)
    if bm is not None:
        eng.set_manager(bm)
    eng.decode_init(m.B, m.P, m.maxT, kv_dtype=hip.HPA_BF16 if m.kv_bf16 else hip.HPA_F32)
    assert eng.free_pages() == m.capacity
    if profile == "chain6":  # the auto form at C = 768 is chain form 6
        plan = hip.layer_plan(1, m.B, m.cfg["C"], m.cfg["NH"], m.maxT, num_cus=hip.device_info()[1])
        assert plan["chain"] == 6 and eng.layer_form() == plan["form"] == 3, (plan, eng.layer_form())
    if m.kv_bf16:  # refused on a bf16 pool, and nothing changed
        with pytest.raises(RuntimeError):
            eng.set_shared_attention(True, min_tiles=1, min_members=2, min_covered=2)
        assert not eng.shared_attention() and eng.free_pages() == m.capacity and not eng.positions().any()
    eng.set_graph(p["graph"])
    if p["shared"]:
        eng.set_shared_attention(True, min_tiles=1, min_members=2, min_covered=2)
    prev = _observe(hip, eng, m, bm)
    worst = dict(logit=0.0, kv=0.0)
    evictions = units = 0
    for i, op in enumerate(trace):
        result = _run(eng, op)
        mask = eng.evicted()
        assert m.evicting or not mask.any(), (profile, seed, i, mask)
        evictions += int(mask.sum())
        exp = m.apply(op, mask if m.evicting else None)
        obs = _observe(hip, eng, m, bm, result)
        w = em.check_op(m, exp, prev, obs, i)
        worst = {k: max(worst[k], w[k]) for k in worst}
        units += bool(obs.plan is not None and obs.plan[0])
        prev = obs
    for b in range(m.B):  # 7. the end of the trace: every page comes back
        eng.release(b)
    assert eng.free_pages() == m.capacity
    assert trace.i == p["n_ops"]
    if p["shared"]:
        assert units, "no op ran with a shared-attention unit live"
    print(f"ENGINETRACE {profile} seed {seed}: {trace.i} ops, worst logit ratio {worst['logit']:.3f} of "
          f"{m.bar:.0e}, worst K/V ratio {worst['kv']:.3f} of {em.KV_RTOL[m.kv_bf16]:.0e}, exempt {m.exempt} / "
          f"{m.picks} picks, {evictions} evictions, {units} ops with a shared unit live, {time.time() - t0:.1f} s")
    eng.close()
    if bm is not None:
        bm.close()
