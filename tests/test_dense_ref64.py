"""tests/dense_ref64.py on the CPU: a numpy fp32 emulation of the dense ragged
pass, clean and with injected faults, through the checker the GPU module
(tests/test_gpu_dense_pass.py) uses, on that module's fp32-weight case tables.

The emulation restates the pass's arithmetic in fp32: every GEMM sums 8 K
ranges (each an fp32 matmul) folded in order, LayerNorm uses one-pass
statistics (sum and sum of squares) over 16-column partial sums -- a single
tile over the whole row at layer 0, where the embedding kernel writes one --
the softmax runs in fp32 over keys 0 .. pos + t of the pool after this pass's
stores, and a bf16 pool stores round-to-nearest-even.  The clean emulation
must pass every check at no more than half of its bar; every mutant must be
rejected by the check named for it:

  attends_next_key / misses_own_key        layer
  wpe_of_neighbour                         embedding
  qkv_ignores_row_seq                      kv: stray and unwritten
  kv_from_neighbour_l1                     kv: value, layer 1 only
  ln_stats_from_first_group                layer, rows 64 and above only
  layer0_reads_all_tiles                   kv: value at layer 0
  gather_next_row                          decode
  score_targets_chunk_off                  score

Worst ratios of the clean emulation (x86-64, numpy; test_clean_emulation
prints them as DENSEEMU lines), against half bars of 2.34e-06 (K/V rows),
2.48e-06 (layer outputs) and 0.5 (logits and scores, as fractions of their
bounds):

  table                          K/V rows   layer outputs  logits  score
  ragged C=768  R=70  P=16       4.3e-07    7.0e-07        0.011   0.004
  ragged C=768  R=90  P=64       4.4e-07    6.6e-07        0.011   0.006
  ragged C=768  R=120 P=8  bf16  1.3e-07    6.4e-07        0.011   0.005
  prefill C=768 3x30  P=16       4.1e-07    6.3e-07        0.017   0.006
  score  C=768  R=90  P=16       4.3e-07    6.3e-07        0.013   0.005
  verify C=768  P=16             3.9e-07    6.5e-07        0.010   0.004
  verify C=768  P=8  bf16        7.3e-08    7.5e-07        0.012   0.004
  ragged C=1024 R=70  P=32       4.5e-07    7.9e-07        0.011   0.004

The same file asserts the input conditions of every GPU case from its lens /
pos tables alone (dense_ref64.case_conditions).
"""
import numpy as np
import pytest

import attn_ref64 as ar
import dense_ref64 as dr
import ref64
from pagedattn import round_bf16
from test_gpu_kv_append import KV_RTOL, OUT_RTOL

L, V = 3, 1000
F, MAX_CTX = dr.F, dr.MAX_CTX

# (name, C, NH, (lens, pos), P, bf16 pool, kind, blocks): the fp32-weight tables of tests/test_gpu_dense_pass.py
TABLES = [
    ("ragged-C768-R70-P16", 768, 12, dr.ragged_case(70, 16), 16, False, "ragged", 5),
    ("ragged-C768-R90-P64", 768, 12, dr.ragged_case(90, 64), 64, False, "ragged", 6),
    ("ragged-C768-R120-P8-bf16pool", 768, 12, dr.ragged_case(120, 8), 8, True, "ragged", 8),
    ("prefill-C768-3x30-P16", 768, 12, dr.prefill_case(30, 16), 16, False, "prefill", 6),
    ("score-C768-R90-P16", 768, 12, dr.ragged_case(90, 16), 16, False, "ragged", 6),
    ("verify-C768-P16", 768, 12, dr.verify_case(16), 16, False, "verify", 2),
    ("verify-C768-P8-bf16pool", 768, 12, dr.verify_case(8), 8, True, "verify", 2),
    ("ragged-C1024-R70-P32", 1024, 16, dr.ragged_case(70, 32), 32, False, "ragged", 5),
]
# tables the bf16-weight GPU cases add (conditions only: the emulation is fp32)
MORE_TABLES = [("ragged-R70-P8", dr.ragged_case(70, 8), 8, "ragged", 5), ("ragged-R130-P8", dr.ragged_case(130, 8), 8, "ragged", 9),
               ("score-R90-P16", dr.ragged_case(90, 16), 16, "ragged", 6)]

_params = {}


def _model(C, NH):
    cfgd = dict(maxT=MAX_CTX, V=V, L=L, NH=NH, C=C)
    if C not in _params:
        _params.clear()  # one model at a time
        _params[C] = ar.peaked_params(cfgd, seed=900 + NH)
    return cfgd, _params[C]


@pytest.fixture(scope="module", autouse=True)
def _drop_params():
    yield
    _params.clear()
    _clean.clear()


# ---------------------------------------------------------------- the fp32 emulation
f32 = np.float32


def _gemm(a, W, bias=None):
    """a (M, K) @ W (N, K).T in fp32: 8 K ranges, folded in order"""
    K = a.shape[1]
    acc = None
    for i in range(8):
        ks = slice(i * K // 8, (i + 1) * K // 8)
        p = np.matmul(a[:, ks], W[:, ks].T, dtype=f32)
        acc = p if acc is None else acc + p
    return acc if bias is None else acc + bias


def _tiles(x):
    """one-pass statistics over 16-column partial sums: (M, C/16, 2) fp32"""
    t = x.reshape(x.shape[0], -1, 16)
    return np.stack([t.sum(-1, dtype=f32), (t * t).sum(-1, dtype=f32)], -1)


def _ln(x, st, w, b):
    """LayerNorm from statistics tiles st (M, ntiles, 2), folded in order"""
    C = x.shape[1]
    s, q = st[:, 0, 0].copy(), st[:, 0, 1].copy()
    for i in range(1, st.shape[1]):
        s, q = s + st[:, i, 0], q + st[:, i, 1]
    mean = s / f32(C)
    var = q / f32(C) - mean * mean
    rstd = (f32(1) / np.sqrt(var + f32(1e-5))).astype(f32)
    return ((x - mean[:, None]) * rstd[:, None] * w + b).astype(f32)


def _gelu(x):
    x = x.astype(f32)
    return (f32(0.5) * x * (f32(1) + np.tanh(f32(ref64.GELU_S) * (x + f32(ref64.GELU_C) * x * x * x)))).astype(f32)


def emulate(ref, tok, lens, pos, pool, kv_bf16=False, mutant=None, last_rows=None, score=None, chunk=32, stale=None):
    """the dense pass in fp32.  pool[l][b] = [K, V] (MAX_CTX, C) fp32, updated in
    place.  score: packed targets (R,) or None.  last_rows: the rows gathered
    (verify), default row0 + len - 1.  Returns dict(xs, logits, next, logprobs, top_ids)."""
    C, NH = ref.C, ref.NH
    B = len(lens)
    R = int(np.sum(lens))
    row0, seq, rpos = dr.row_tables(lens, pos)
    p = ref
    epos = rpos.copy()
    if mutant == "wpe_of_neighbour":
        epos[20] = rpos[21]
    x = (p.wte[np.asarray(tok)] + p.wpe[epos]).astype(f32)
    st = np.stack([x.sum(-1, dtype=f32), (x * x).sum(-1, dtype=f32)], -1)[:, None, :]  # one tile
    if mutant == "layer0_reads_all_tiles":  # tile 0 as written, the other C/16 - 1 as an earlier pass left them
        st = np.concatenate([st, stale[:R, 1:]], 1)
    xs = [x]
    for l in range(ref.L):
        a = _ln(x, st, p._layer(2, l, C), p._layer(3, l, C))
        a_kv = a
        if mutant == "kv_from_neighbour_l1" and l == 1:
            nb = np.arange(R) ^ 1
            a_kv = a[np.where(nb < R, nb, np.arange(R))]
        Wq = p._layer(4, l, (3 * C, C))
        bq = p._layer(5, l, 3 * C)
        q = _gemm(a, Wq[:C], bq[:C])
        kv = _gemm(a_kv, Wq[C:], bq[C:])
        if kv_bf16:
            kv = round_bf16(kv)
        for r in range(R):
            b = r % B if mutant == "qkv_ignores_row_seq" else seq[r]
            pool[l][b][0][rpos[r]] = kv[r, :C]
            pool[l][b][1][rpos[r]] = kv[r, C:]
        att = np.zeros((R, C), f32)
        for r in range(R):
            n = int(rpos[r]) + 1
            if mutant == "attends_next_key":
                n = min(n + 1, MAX_CTX)
            elif mutant == "misses_own_key":
                n = max(n - 1, 1)
            Kb = pool[l][seq[r]][0][:n].reshape(n, NH, 64)
            Vb = pool[l][seq[r]][1][:n].reshape(n, NH, 64)
            s = np.einsum("hd,thd->ht", q[r].reshape(NH, 64), Kb).astype(f32) * f32(0.125)
            e = np.exp(s - s.max(-1, keepdims=True)).astype(f32)
            w = e / e.sum(-1, keepdims=True, dtype=f32)
            att[r] = np.einsum("ht,thd->hd", w, Vb).astype(f32).reshape(C)
        res2 = x + _gemm(att, p._layer(6, l, (C, C)), p._layer(7, l, C))
        st2 = _tiles(res2)
        if mutant == "ln_stats_from_first_group":
            st2[64:] = st2[:R - 64]
        h = _gelu(_gemm(_ln(res2, st2, p._layer(8, l, C), p._layer(9, l, C)), p._layer(10, l, (4 * C, C)),
                        p._layer(11, l, 4 * C)))
        x = (res2 + _gemm(h, p._layer(12, l, (C, 4 * C)), p._layer(13, l, C))).astype(f32)
        st = _tiles(x)
        xs.append(x)
    xs = np.stack(xs)
    out = dict(xs=xs)
    xf = _ln(x, st, p._t(14), p._t(15))
    all_logits = _gemm(xf, p.wte)  # what each row's LOGITS / SCORE GEMM sees
    last = row0 + np.asarray(lens) - 1 if last_rows is None else np.asarray(last_rows).copy()
    if mutant == "gather_next_row":
        last = last + 1
    padded = np.concatenate([all_logits, _gemm(_ln(np.zeros((1, C), f32), np.zeros((1, 1, 2), f32), p._t(14), p._t(15)),
                                               p.wte)])  # row R: a zero padded row
    out["logits"] = np.stack([padded[min(max(last[b], 0), R)] for b in range(B)])
    out["next"] = out["logits"].argmax(-1)
    out["top_ids"] = all_logits.argmax(-1)
    if score is not None:
        tgt = np.asarray(score).copy()
        if mutant == "score_targets_chunk_off":
            tgt[chunk:2 * chunk] = np.resize(np.asarray(score)[2 * chunk:], chunk)  # what lies one chunk further on
        x64 = all_logits.astype(np.float64)
        m = x64.max(-1, keepdims=True)
        lse = (m + np.log(np.exp(x64 - m).sum(-1, keepdims=True)))[:, 0]
        out["logprobs"] = np.where(tgt < 0, 0.0, x64[np.arange(R), np.where(tgt < 0, 0, tgt)] - lse).astype(f32)
    return out


class Scene:
    """one case table: the pool as fill_random would leave it (random rows
    [0, F), zeros after), tokens, and the emulated pass"""

    def __init__(self, name, C, NH, table, P, kv_bf16, kind, blocks):
        self.name, self.kind, self.kv_bf16 = name, kind, kv_bf16
        self.lens, self.pos = table
        cfgd, params = _model(C, NH)
        self.ref = ref64.Ref64(cfgd, params, kv_bf16=kv_bf16)
        self.rng = np.random.default_rng(len(name) + C)
        self.B, self.R = len(self.lens), int(self.lens.sum())
        self.tok = self.rng.integers(0, V, self.R)
        st = round_bf16 if kv_bf16 else (lambda a: a)
        self.pool0 = [[[np.concatenate([st(self.rng.uniform(-1, 1, (F, C)).astype(f32)), np.zeros((MAX_CTX - F, C), f32)])
                        for _ in "KV"] for _ in range(self.B)] for _ in range(L)]
        self.stale = _tiles(self.rng.uniform(-1, 1, (self.R, C)).astype(f32))
        self.n_after = np.maximum(self.pos + self.lens, F)
        row0 = dr.row_tables(self.lens, self.pos)[0]
        self.targets = self.rng.integers(0, V, self.R).astype(np.int32)
        self.targets[row0[self.lens > 0] + self.lens[self.lens > 0] - 1] = -1  # the last row of a sequence: no target
        # verify: the accepted row is some row of the sequence, not always the last
        self.last_rows = row0 + np.array([-1, 0, 1, 2, 7, 3, 0])[:self.B] if kind == "verify" else None

    def run(self, mutant=None):
        pool = [[[a.copy() for a in kv] for kv in layer] for layer in self.pool0]
        out = emulate(self.ref, self.tok, self.lens, self.pos, pool, self.kv_bf16, mutant, self.last_rows,
                      self.targets, stale=self.stale)
        before = [[tuple(a[:F] for a in kv) for kv in layer] for layer in self.pool0]
        after = [[tuple(a[:self.n_after[b]] for a in layer[b]) for b in range(self.B)] for layer in pool]
        score = dict(targets=self.targets, logprobs=out["logprobs"], top_ids=out["top_ids"])
        return dr.check_pass(self.ref, self.tok, self.lens, self.pos, out["xs"], before, after, KV_RTOL[False],
                             OUT_RTOL[False], logits=out["logits"], next_ids=out["next"], last_rows=self.last_rows,
                             score=score, collect=True)


_clean = {}


def _scene(i):
    if i not in _clean:
        for k in [k for k in _clean if TABLES[k][1] != TABLES[i][1]]:
            del _clean[k]
        _clean[i] = Scene(*TABLES[i])
    return _clean[i]


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("i", range(len(TABLES)), ids=[t[0] for t in TABLES])
def test_case_conditions(i):
    name, C, NH, (lens, pos), P, _, kind, blocks = TABLES[i]
    dr.case_conditions(lens, pos, P, blocks, kind)


@pytest.mark.parametrize("name,table,P,kind,blocks", MORE_TABLES, ids=[t[0] for t in MORE_TABLES])
def test_case_conditions_bf16_weight_tables(name, table, P, kind, blocks):
    dr.case_conditions(table[0], table[1], P, blocks, kind)


def test_case_conditions_reject():
    """the conditions are assertions: tables that miss one are refused"""
    lens, pos = dr.ragged_case(70, 16)
    with pytest.raises(AssertionError):
        dr.case_conditions(lens, pos, 16, 4)  # named for the wrong row-block count
    with pytest.raises(AssertionError):
        dr.case_conditions(lens, np.where(pos == 0, 1, pos), 16, 5)  # nobody starts at 0
    with pytest.raises(AssertionError):
        dr.case_conditions(np.where(lens == 0, 2, lens), pos, 16, 5)  # no empty sequence
    with pytest.raises(AssertionError):
        dr.case_conditions(lens, np.where(pos == F, F + 60, pos), 16, 5)  # past MAX_CTX
    score = dr.ragged_case(90, 16)[0].sum()
    assert score % 32 == 26  # set_score_chunk(32): a last chunk of 26 rows


@pytest.mark.parametrize("i", range(len(TABLES)), ids=[t[0] for t in TABLES])
def test_clean_emulation(i):
    """a correct fp32 pass: every check at no more than half of its bar"""
    ratios, failures = _scene(i).run()
    assert not failures, failures
    print(f"DENSEEMU {TABLES[i][0]} kv={ratios['kv']:.3e} out={ratios['layer']:.3e} logits={ratios['decode']:.3f} "
          f"score={ratios['score']:.3f}")
    assert ratios["embedding"] == 0.0
    assert ratios["kv"] <= 0.5 * KV_RTOL[False], ratios
    assert ratios["layer"] <= 0.5 * OUT_RTOL[False], ratios
    assert ratios["decode"] <= 0.5 and ratios["score"] <= 0.5, ratios


def _mutant(i, name):
    ratios, failures = _scene(i).run(name)
    return _scene(i), ratios, failures


@pytest.mark.parametrize("mutant", ["attends_next_key", "misses_own_key"])
def test_mutant_causal_mask(mutant):
    s, _, failures = _mutant(0, mutant)
    assert "layer" in failures and "embedding" not in failures and "kv" not in failures
    assert failures["layer"].layers == [0, 1, 2]


def test_mutant_wpe_of_neighbour():
    _, _, failures = _mutant(0, "wpe_of_neighbour")
    assert failures["embedding"].rows == [20]


def test_mutant_qkv_ignores_row_seq():
    s, _, failures = _mutant(0, "qkv_ignores_row_seq")
    kinds = {f[5] for f in failures["kv"].faults}
    assert {"stray", "unwritten"} <= kinds
    assert {f[0] for f in failures["kv"].faults} == {0, 1, 2}
    assert any(f[1] == 0 and f[5] == "stray" for f in failures["kv"].faults)  # the sequence of no rows was written to


def test_mutant_kv_from_neighbour_at_layer_1():
    _, _, failures = _mutant(0, "kv_from_neighbour_l1")
    faults = failures["kv"].faults
    assert {f[0] for f in faults} == {1} and {f[5] for f in faults} == {"value"}
    assert "embedding" not in failures


def test_mutant_ln_stats_from_first_row_group():
    s, _, failures = _mutant(0, "ln_stats_from_first_group")
    assert s.R > 64
    rows = failures["layer"].rows
    assert rows and min(rows) >= 64
    assert "kv" not in failures and "embedding" not in failures


def test_mutant_layer0_reads_all_tiles():
    _, _, failures = _mutant(0, "layer0_reads_all_tiles")
    faults = failures["kv"].faults
    assert {f[0] for f in faults} == {0} and {f[5] for f in faults} == {"value"}
    assert "embedding" not in failures


@pytest.mark.parametrize("i", [0, 5], ids=["ragged", "verify"])
def test_mutant_gather_next_row(i):
    _, _, failures = _mutant(i, "gather_next_row")
    assert set(failures) == {"decode"}
    assert len(failures["decode"].rows) >= 3


def test_mutant_score_targets_chunk_off():
    s, _, failures = _mutant(4, "score_targets_chunk_off")
    assert set(failures) == {"score"}
    assert set(failures["score"].rows) <= set(range(32, 64)) and len(failures["score"].rows) >= 16
