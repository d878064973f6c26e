"""Engine-level speculative greedy decoding: gpt2_decode_verify against the
oracle's token-by-token greedy stream.

Model: SMALL of tests/test_gpu_score.py, synth.params(SMALL, seed=11), B = 4,
page 16.  Ground truth: oc.PagedDecoder fed 9 forced tokens per sequence
(default_rng(5).integers(0, 1000, (9, 4))) and then its own greedy ids for 64
steps.  STREAM[t][b] is sequence b's t-th greedy id (STREAM[0] is pending after
the forced tokens), LOGITS[t][b] the logits it is the argmax of.

No row is left out: the oracle's top-2 margin is asserted to clear MIN_MARGIN >
TIE_MARGIN on every row of the 64 steps (fp32), so ids are compared exactly.
The stream repeats tokens heavily (transitions at steps 7 and 12 of sequence
0, 1 of sequence 1, 7 and 18 of sequence 2), so the full-acceptance test
counts the accepted drafts that differ from the token before them and asserts
at least 4: a row-alignment bug cannot hide behind repetition.

Bars: LOGIT_TOL = 2e-4 on logits (tests/test_gpu_prefill.py's), 2 * LOGIT_TOL
on log-probabilities (a sup-norm logit error eps moves the target's logit and
the log-sum-exp by at most eps each); bf16: the bars of
test_score_matches_oracle_bf16_weights (2e-2, tie 4e-2)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
import score_ref64 as sr
import synth
from test_gpu_kv_append import KV_RTOL
from test_gpu_score import LOGIT_TOL, SMALL, TIE_MARGIN, V

pytestmark = pytest.mark.gpu
B, P, PRE, STEPS = 4, 16, 9, 64
MIN_MARGIN = 2.2e-3
MR = 8  # HPA_VERIFY_MAX_ROWS
_I = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def params():
    return synth.params(SMALL, seed=11)


def _forced():
    return np.random.default_rng(5).integers(0, 1000, (PRE, B)).astype(np.int32)


class _Truth:
    """the oracle's greedy run; the decoder stays open (get_kv of any prefix)"""

    def __init__(self, params, bf16=False):
        c = oc.cfg(SMALL["maxT"], V, SMALL["L"], SMALL["NH"], SMALL["C"])
        self.orc = oc.PagedDecoder(params, c, B, P, SMALL["maxT"], kv_bf16=bf16, w_bf16=bf16)
        pre = _forced()
        for t in range(PRE):
            nxt, lg = self.orc.step(pre[t])
        self.stream = np.zeros((STEPS, B), np.int32)
        self.logits = np.zeros((STEPS, B, V), np.float32)
        for t in range(STEPS):
            self.stream[t], self.logits[t] = nxt, lg
            nxt, lg = self.orc.step(nxt)
        s = np.sort(self.logits, -1)
        self.margin = s[..., -1] - s[..., -2]  # (STEPS, B)

    def close(self):
        self.orc.close()


@pytest.fixture(scope="module")
def truth(params):
    t = _Truth(params)
    # the condition under which ids are compared exactly, from the oracle alone
    assert t.margin.min() >= MIN_MARGIN > TIE_MARGIN, t.margin.min()
    assert np.array_equal(sr.first_argmax(t.logits.reshape(-1, V)).reshape(STEPS, B), t.stream)
    yield t
    t.close()


def _model(hip, params, s=0, stream=None, **kw):
    """an engine after the forced tokens and s greedy steps (pending: stream[s])"""
    m = hip.Model(SMALL, params=params)
    m.decode_init(B, P, SMALL["maxT"], **kw)
    pre = _forced()
    for t in range(PRE):
        nxt = m.step(pre[t])
    for t in range(s):
        assert np.array_equal(nxt, stream[t])
        nxt = m.step(None)
    if stream is not None:
        assert np.array_equal(nxt, stream[s])
    return m


def _pending(hip, m):
    out = np.zeros(m.B, np.int32)
    hip.check(hip.lib().hpa_memcpy(out.ctypes.data, m.next_ptr(), out.nbytes), "next ids")
    return out


def _teacher_forced(params, s_of, fed, stream, bf16=False):
    """the oracle's logits after each fed token: sequence b is first advanced
    to greedy step s_of[b] (forced tokens, then its own stream), then fed
    fed[b][0], fed[b][1], ...; returns per sequence (len(fed[b]), V)"""
    out = []
    c = oc.cfg(SMALL["maxT"], V, SMALL["L"], SMALL["NH"], SMALL["C"])
    pre = _forced()
    for b in range(B):  # one single-sequence oracle each: the sequences stand at different steps
        o = oc.PagedDecoder(params, c, 1, P, SMALL["maxT"], page_seed=b + 1, kv_bf16=bf16, w_bf16=bf16)
        for t in range(PRE):
            o.step(pre[t, b:b + 1])
        for t in range(s_of[b]):
            o.step(stream[t, b:b + 1])
        rows = np.zeros((len(fed[b]), V), np.float32)
        for i, tok in enumerate(fed[b]):
            rows[i] = o.step(np.array([tok], np.int32))[1][0]
        o.close()
        out.append(rows)
    return out


def test_oracle_drafts_are_all_accepted(hip, params, truth):
    """drafts = the oracle's continuation, k = 7, 3, 1, 0 rotated over the batch
    for four consecutive passes; the accepted row's logits and the pending
    token's log-probability against the oracle's"""
    m = _model(hip, params, 0, truth.stream)
    m.set_logprobs(True)
    assert hip.verify_plan(8, hip.HPA_F32, P) == 1
    s = np.zeros(B, int)
    changed = 0
    worst = 0.0
    for ks in ([7, 3, 1, 0], [7, 0, 7, 3], [0, 1, 3, 7], [3, 0, 7, 1]):
        drafts = [truth.stream[s[b] + 1:s[b] + 1 + ks[b], b].tolist() for b in range(B)]
        pos0 = m.positions()
        acc, toks, _ = m.verify(drafts)
        for b in range(B):
            assert acc[b] == ks[b], (b, acc, ks)
            assert toks[b] == truth.stream[s[b] + 1:s[b] + ks[b] + 2, b].tolist(), b
            prev = truth.stream[s[b]:s[b] + ks[b], b]
            changed += int((np.asarray(drafts[b], np.int32) != prev).sum())
        s += np.asarray(ks) + 1
        assert np.array_equal(m.positions(), pos0 + np.asarray(ks) + 1)
        assert np.array_equal(_pending(hip, m), truth.stream[s, np.arange(B)])
        lg, lp = m.logits(), m.logprobs()
        for b in range(B):
            worst = max(worst, float(np.abs(lg[b] - truth.logits[s[b], b]).max()))
            ref = sr.logprob64(truth.logits[s[b], b][None], truth.stream[s[b], b:b + 1])[0]
            assert abs(lp[b] - ref) <= 2 * LOGIT_TOL, (b, lp[b], ref)
    print(f"SPEC full acceptance: worst |logit diff| {worst:.3e} (bar {LOGIT_TOL:.1e}), "
          f"{changed} accepted drafts differ from the token before them")
    assert changed >= 4
    assert worst <= LOGIT_TOL
    # decoding goes on from the verified state
    for t in range(3):
        assert np.array_equal(m.step(None), truth.stream[s + 1 + t, np.arange(B)])
    m.close()


@pytest.mark.parametrize("j", range(7))
def test_first_wrong_draft_stops_acceptance(hip, params, truth, j):
    """entry j of each sequence's drafts replaced by (id + 1) % V (sequences
    with k <= j keep the oracle's drafts): n_accepted = j there"""
    s0 = 5  # drafts of sequence 0 cross its transition at step 7, of sequence 2 too
    m = _model(hip, params, s0, truth.stream)
    ks = [7, 3, 7, 1]
    drafts = [truth.stream[s0 + 1:s0 + 1 + ks[b], b].copy() for b in range(B)]
    want = list(ks)
    for b in range(B):
        if j < ks[b]:
            drafts[b][j] = (drafts[b][j] + 1) % V
            want[b] = j
    pos0 = m.positions()
    acc, toks, _ = m.verify([d.tolist() for d in drafts])
    assert acc == want
    for b in range(B):
        assert toks[b] == truth.stream[s0 + 1:s0 + want[b] + 2, b].tolist(), b
    assert np.array_equal(m.positions(), pos0 + np.asarray(want) + 1)
    m.close()


def test_draft_logprobs_teacher_forced(hip, params, truth):
    """random drafts: every drafted row's log-probability against the oracle fed
    the same drafted tokens, accepted or not"""
    s0 = 3
    m = _model(hip, params, s0, truth.stream)
    rng = np.random.default_rng(21)
    ks = [7, 4, 1, 6]
    drafts = [rng.integers(0, V, k).astype(np.int32) for k in ks]
    drafts[1][0] = truth.stream[s0 + 1, 1]  # one accepted draft ahead of rejected ones
    acc, toks, lps = m.verify([d.tolist() for d in drafts], want_logprobs=True)
    fed = [[int(truth.stream[s0, b])] + drafts[b].tolist() for b in range(B)]
    rows = _teacher_forced(params, [s0] * B, fed, truth.stream)
    worst = 0.0
    for b in range(B):
        ref = sr.logprob64(rows[b][:ks[b]], drafts[b])
        worst = max(worst, float(np.abs(lps[b] - ref).max()))
        # acceptance follows the teacher-forced argmax where it is clear
        srt = np.sort(rows[b], -1)
        clear = srt[:, -1] - srt[:, -2] > TIE_MARGIN
        a = 0
        while a < ks[b] and clear[a] and sr.first_argmax(rows[b][a:a + 1])[0] == drafts[b][a]:
            a += 1
        if clear[:a + 1].all():
            assert acc[b] == a, (b, acc[b], a)
            assert toks[b][-1] == sr.first_argmax(rows[b][a:a + 1])[0]
    assert acc[1] >= 1
    print(f"SPEC draft logprobs: worst |diff| {worst:.3e} (bar {2 * LOGIT_TOL:.1e})")
    assert worst <= 2 * LOGIT_TOL
    m.close()


def test_stale_slots_are_never_read(hip, params, truth):
    """a pass from position 13 whose rejected rows spill into a fresh page
    (positions 13..20, page edge at 16), then 12 decode steps and the K/V of
    every position against the oracle's"""
    s0 = 4
    m = _model(hip, params, s0, truth.stream)
    assert (m.positions() == 13).all()
    want = [1, 0, 3, 7]
    drafts = [truth.stream[s0 + 1:s0 + 8, b].copy() for b in range(B)]
    for b in range(B):
        if want[b] < 7:
            drafts[b][want[b]] = (drafts[b][want[b]] + 1) % V
    acc, toks, _ = m.verify([d.tolist() for d in drafts])
    assert acc == want
    s = s0 + np.asarray(want) + 1
    for t in range(12):
        assert np.array_equal(m.step(None), truth.stream[s + 1 + t, np.arange(B)]), t
    pos = m.positions()
    assert np.array_equal(pos, PRE + s + 12)
    worst = 0.0
    for l in range(SMALL["L"]):
        for b in range(B):
            k, v = m.read_kv(l, b, int(pos[b]))
            ko, vo = truth.orc.get_kv(l, b, int(pos[b]))
            for got, ref in ((k, ko), (v, vo)):
                r = np.abs(got.astype(np.float64) - ref).max(-1) / np.abs(ref).max(-1)
                worst = max(worst, float(r.max()))
    print(f"SPEC stale slots: worst K/V row ratio {worst:.3e} (bar {KV_RTOL[False]:.2e})")
    assert worst <= KV_RTOL[False]
    m.close()


def test_untouched_sequences(hip, params, truth):
    """n_draft = -1: position, pending id, logits row (bitwise) and
    log-probability unchanged while the other sequences advance"""
    s0 = 2
    m = _model(hip, params, s0, truth.stream)
    m.set_logprobs(True)
    m.step(None)  # a pick with log-probabilities on
    s0 += 1
    pos0, pend0, lg0, lp0 = m.positions(), _pending(hip, m), m.logits(), m.logprobs()
    drafts = [truth.stream[s0 + 1:s0 + 4, 0].tolist(), None, [], None]
    acc, toks, lps = m.verify(drafts, want_logprobs=True)
    assert acc == [3, None, 0, None] and toks[1] is None and lps[3] is None
    assert toks[0] == truth.stream[s0 + 1:s0 + 5, 0].tolist() and toks[2] == [int(truth.stream[s0 + 1, 2])]
    pos, pend, lg, lp = m.positions(), _pending(hip, m), m.logits(), m.logprobs()
    assert np.array_equal(pos, pos0 + [4, 0, 1, 0])
    for b in (1, 3):
        assert pend[b] == pend0[b]
        assert np.array_equal(lg[b].view(np.int32), lg0[b].view(np.int32))
        assert lp[b].view(np.int32) == lp0[b].view(np.int32)
    assert pend[0] == truth.stream[s0 + 4, 0] and pend[2] == truth.stream[s0 + 1, 2]
    # all untouched: nothing moves
    acc, toks, _ = m.verify([None] * B)
    assert acc == [None] * B and np.array_equal(m.positions(), pos)
    # the untouched sequences decode on as if nothing had happened
    nxt = m.step(None)
    assert nxt[1] == truth.stream[s0 + 1, 1] and nxt[3] == truth.stream[s0 + 1, 3]
    m.close()


def test_prefill_kernel_route_is_equivalent(hip, params, truth):
    """request 1 (the MFMA prefill kernel) against auto (the verify kernel)"""
    s0 = 5
    outs = []
    for request in (0, 1):
        m = _model(hip, params, s0, truth.stream)
        m.set_verify_attention(request)
        drafts = [truth.stream[s0 + 1:s0 + 8, b].copy() for b in range(B)]
        drafts[1][2] = (drafts[1][2] + 1) % V
        acc, toks, _ = m.verify([d.tolist() for d in drafts])
        outs.append((acc, toks, m.logits()))
        m.close()
    assert outs[0][0] == outs[1][0] == [7, 2, 7, 7]
    assert outs[0][1] == outs[1][1]
    d = float(np.abs(outs[0][2] - outs[1][2]).max())
    print(f"SPEC routes: |logit diff| {d:.3e}")
    assert d <= 2 * LOGIT_TOL


def test_bf16_pool_takes_the_prefill_kernel(hip, params):
    """bf16 weights and KV pool: the plan reports 0 and the pass works.  The
    window is greedy steps 8..16 (the pending id and k = 7 drafts for every
    sequence): the oracle's bf16 margins clear 4e-2 on each of its rows,
    asserted here (the steps before it do not: they are fed, not picked)"""
    tol, tie, s0, k = 2e-2, 4e-2, 8, 7
    t = _Truth(params, bf16=True)
    try:
        assert t.margin[s0:s0 + k + 2].min() > tie, t.margin[s0:s0 + k + 2].min()
        assert hip.verify_plan(k + 1, hip.HPA_BF16, P) == 0 and hip.verify_plan(k + 1, hip.HPA_BF16, P, request=2) == 0
        m = hip.Model(SMALL, params=params)
        m.decode_init(B, P, SMALL["maxT"], kv_dtype=hip.HPA_BF16, w_dtype=hip.HPA_BF16)
        pre = _forced()
        for i in range(PRE):
            m.step(pre[i])
        m.prefill_ragged([t.stream[:s0, b] for b in range(B)])  # the oracle's ids, whatever the engine would pick
        drafts = [t.stream[s0 + 1:s0 + 1 + k, b].tolist() for b in range(B)]
        # pending: the engine's own pick after the last fed id; the window's margins make it the oracle's
        assert np.array_equal(_pending(hip, m), t.stream[s0])
        acc, toks, _ = m.verify(drafts)
        assert acc == [k] * B
        for b in range(B):
            assert toks[b] == t.stream[s0 + 1:s0 + k + 2, b].tolist()
        d = float(np.abs(m.logits() - t.logits[s0 + k + 1]).max())
        print(f"SPEC bf16: |logit diff| {d:.3e} (bar {tol:.0e})")
        assert d <= tol
        m.close()
    finally:
        t.close()


def test_forked_pair(hip, params, truth):
    """verify a source and its fork in one pass: the fork's rejected rows land
    in its private tail page, the source's K/V is unchanged"""
    s0 = 11  # position 20: one full shared page, four tokens in the copied tail
    m = hip.Model(SMALL, params=params)
    m.decode_init(2, P, SMALL["maxT"])
    seq0 = np.concatenate([_forced()[:, 0], truth.stream[:s0, 0]])
    nxt = m.prefill_ragged([seq0, []])
    assert nxt[0] == truth.stream[s0, 0]
    m.fork(0, 1)
    before = [m.read_kv(l, 0, PRE + s0) for l in range(SMALL["L"])]
    good = truth.stream[s0 + 1:s0 + 8, 0]
    bad = good.copy()
    bad[0] = (bad[0] + 1) % V
    acc, toks, _ = m.verify([good[:3].tolist(), bad.tolist()])
    assert acc == [3, 0]
    assert toks[0] == truth.stream[s0 + 1:s0 + 5, 0].tolist() and toks[1] == [int(truth.stream[s0 + 1, 0])]
    assert np.array_equal(m.positions(), [PRE + s0 + 4, PRE + s0 + 1])
    for l in range(SMALL["L"]):
        k, v = m.read_kv(l, 0, PRE + s0)
        assert np.array_equal(k.view(np.int32), before[l][0].view(np.int32))
        assert np.array_equal(v.view(np.int32), before[l][1].view(np.int32))
    for t in range(4):  # both go on along the same stream, three tokens apart
        nxt = m.step(None)
        assert nxt[0] == truth.stream[s0 + 5 + t, 0] and nxt[1] == truth.stream[s0 + 2 + t, 0]
    m.close()


def _raw_verify(hip, m, drafts, nd):
    drafts = np.ascontiguousarray(drafts, np.int32)
    nd = np.ascontiguousarray(nd, np.int32)
    acc = np.full(len(nd), -7, np.int32)
    toks = np.zeros((len(nd), MR), np.int32)
    return hip.lib().gpt2_decode_verify(m.h, drafts.ctypes.data_as(_I), nd.ctypes.data_as(_I),
                                        acc.ctypes.data_as(_I), toks.ctypes.data_as(_I), None)


def test_refusals_change_nothing(hip, params, truth):
    m = hip.Model(SMALL, params=params)
    m.decode_init(B, P, 16)  # max_ctx 16: position 9 + 8 rows overflows
    pre = _forced()
    for t in range(PRE):
        m.step(pre[t])
    pos0, pend0 = m.positions(), _pending(hip, m)
    ok = truth.stream[1:8, 0]

    def unchanged():
        return np.array_equal(m.positions(), pos0) and np.array_equal(_pending(hip, m), pend0)

    assert _raw_verify(hip, m, np.tile(ok, 4), [7, 7, 7, 7]) != 0 and unchanged()       # 9 + 8 > max_ctx
    assert _raw_verify(hip, m, np.tile(ok, 4), [8, 0, 0, 0]) != 0 and unchanged()       # n_draft > 7
    assert _raw_verify(hip, m, ok, [-2, 0, 0, 0]) != 0 and unchanged()                  # n_draft < -1
    assert _raw_verify(hip, m, [1, V, 2], [3, 0, 0, -1]) != 0 and unchanged()           # id == V
    assert _raw_verify(hip, m, [1, -1, 2], [0, 3, 0, -1]) != 0 and unchanged()          # id < 0
    for filtered in (False, True):                                                      # sampling modes 1 and 2
        m.set_sampling(True, seed=3, filtered=filtered)
        assert _raw_verify(hip, m, ok[:2], [2, 0, 0, 0]) != 0 and unchanged()
    m.set_sampling(False)
    assert _raw_verify(hip, m, ok[:6], [6, 0, 0, -1]) == 0  # 9 + 7 rows fills the context exactly: accepted
    assert np.array_equal(m.positions(), pos0 + [7, 1, 1, 0])
    m.close()
    fresh = hip.Model(SMALL, params=params)  # no engine
    assert _raw_verify(hip, fresh, ok[:2], [2, 0, 0, 0]) != 0
    fresh.close()


def test_c_driver_speculate_prints_the_same_ids(hip, params, truth, tmp_path):
    """examples/decode_main.c -g with and without --speculate 4 on a checkpoint
    of the small model, the forced tokens as the prompt, 40 new tokens: the
    same ids (the oracle's stream, whose margins clear TIE_MARGIN on every one
    of these steps) and the same printed text; one closing line more"""
    N = 40
    assert truth.margin[:N].min() > TIE_MARGIN
    libdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm.c-paged_amd")
    repo = os.path.dirname(libdir)
    exe = str(tmp_path / "decode_main")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", os.path.join(repo, "examples", "decode_main.c"),
                    "-I" + os.path.join(repo, "include"), "-L" + libdir, "-lpaged_hip", "-Wl,-rpath," + libdir,
                    "-o", exe], check=True)
    ck = str(tmp_path / "small.bin")
    synth.write_checkpoint(ck, SMALL, params)
    tok = tmp_path / "prompt.bin"
    np.ascontiguousarray(_forced().T).tofile(tok)  # (B, PRE): sequence-major
    outs = []
    for extra in ([], ["--speculate", "4"]):
        ids = tmp_path / f"ids{len(extra)}.bin"
        r = subprocess.run([exe, "-c", ck, "-t", str(tok), "-b", str(B), "-p", str(PRE), "-n", str(N), "-g",
                            "-o", str(ids)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append((np.fromfile(ids, np.int32).reshape(B, PRE + N), r.stdout))
    (plain, text0), (spec, text1) = outs
    assert np.array_equal(plain[:, PRE:], truth.stream[:N].T)
    assert np.array_equal(spec, plain)

    def printed(text):  # the ids of sequence 0 between the rulers
        return text.split("generating:\n---\n")[1].split("\n---\nFinished!")[0]

    assert printed(text0) == printed(text1) == "".join(f"{t} " for t in plain[0, PRE:])
    line = [ln for ln in text1.splitlines() if ln.startswith("speculation:")]
    assert len(line) == 1 and "speculation:" not in text0
    passes, tokens = int(line[0].split()[1]), int(line[0].split()[3])
    assert tokens == B * (N - 1) and passes < N - 1, line  # the repetitive stream is drafted well: fewer passes than steps
    # sampling flags and --speculate do not combine
    for bad in (["--speculate", "4"], ["-g", "--speculate", "4", "--top-k", "5"], ["-g", "--speculate", "8"]):
        r = subprocess.run([exe, "-c", ck, "-b", "1", "-p", "2", "-n", "2"] + bad, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "speculate" in r.stderr, bad
