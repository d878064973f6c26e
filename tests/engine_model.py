"""A float64 model of the decode engine's state, a random op generator driven
by it, and the checker that holds the engine to it after every call.

Numpy only: no GPU, no oracle.  At any moment each slot of the engine is a
token history, and everything the engine reports for the slot follows from
it: the logits row is the float64 forward of the history, the pending id its
argmax, the K/V rows those of the history's tokens, the pages what the
header's rules (include/paged_infer.h) say the calls so far took and shared.

  Decoder64     an incremental float64 decoder on ref64.Ref64 (per-layer K/V,
                feed / fork / rewind)
  EngineModel   the expected state of B slots: history, decoder, pending id,
                the float64 row of the last fed token, abstract page lists
  Trace         make_trace(profile, seed, n_ops): a deterministic op generator
                that reads nothing but the model, so any prefix of a trace is
                a trace and a failure at op i reproduces with n_ops = i + 1
  check_op      what the engine reported after one op against the model and
                against what it reported before the op

The driver (tests/test_gpu_engine_traces.py on the card, tests/
test_engine_model.py with the model's own values) runs, per op,

    exp = model.apply(op)            # the model moves, and says what to expect
    obs = <observe the engine>       # or model.observe()
    check_op(model, exp, prev, obs)  # raises CheckFailed(check, slot, ...)

Bars: the project's engine bars (tests/test_gpu_serving.py, test_gpu_fork.py,
test_gpu_decode.py): |logit - float64 logit| <= 2e-4 with an fp32 pool, 5e-3
with a bf16 pool.  A greedy id is held to the float64 argmax where the
float64 top-2 margin exceeds 2 x bar (two rows within bar of one another
cannot order two such columns differently); below that the row is "exempt":
the engine's id must still be the first argmax of its own row, and the model
adopts it as the slot's pending id.

K/V rows written by a pass are held to the float64 rows at KV_RTOL x max|row|
(+ half a bf16 ulp in a bf16 pool).  The engine's layer bar is
FP32_LAYER_RTOL = 1e-5 x max|x| per layer (tests/test_gpu_configs.py); a K/V
row of layer l is a linear map of LN1(x_l), x_l carries l layers of that bar
and the row its own, and LayerNorm scales an error relative to max|x| by at
most max|x| / rms(x) (below 5 for these weights): 5 x L x 1e-5 = 1e-4 for the
two-layer configs here.  A bf16 pool's rows are computed in fp32 from a
context of bf16 keys, which both sides round alike up to single flips of one
ulp (2^-8) in a few of the C products of a score: BF16_LAYER_RTOL = 4e-3, the
project's bar for that regime, taken once.  A row of the wrong token or the
wrong position is off by a ratio of order 1.  KV_RTOL is a NEW bar of this
file, not one of the project's: the per-kernel files hold a K/V row to 1e-5
or less on the kernel's own inputs, here the inputs are the engine's own
earlier outputs; the engine measures about 1 % of it, and bit identity
(checks 3 and 4) guards everything a pass must not write.
"""
import zlib

import numpy as np

import ref64
import synth
import tree_ref64 as tr

SMALL = dict(maxT=256, V=1000, L=2, NH=2, C=128)
CHAIN = dict(maxT=256, V=1000, L=2, NH=12, C=768)
LOGIT_TOL = 2e-4        # tests/test_gpu_serving.py, test_gpu_fork.py, test_gpu_decode.py
BF16_LOGIT_TOL = 5e-3   # tests/test_gpu_decode.py
KV_RTOL = {False: 1e-4, True: 4e-3}  # keyed by kv_bf16; the module docstring derives them
MR = tr.MR

# kinds of op a trace may hold; "admit" and "ragged" are both one gpt2_decode_prefill_ragged call
FULL_KINDS = ("admit", "ragged", "step_host", "step_dev", "verify", "verify_tree", "fork", "release", "rewind",
              "reserve", "reset", "set_graph", "set_shared", "set_verify_attention", "set_attn_splits")
PROFILES = {
    "f32-all": dict(cfg=SMALL, kv_bf16=False, B=6, P=16, n_ops=80, seeds=(1, 2, 3), bar=LOGIT_TOL, graph=False,
                    shared=False, manager=None, kinds=FULL_KINDS),
    "f32-shared-graph": dict(cfg=SMALL, kv_bf16=False, B=6, P=8, n_ops=80, seeds=(1, 2), bar=LOGIT_TOL, graph=True,
                             shared=True, manager="full", kinds=FULL_KINDS),
    "bf16-pool": dict(cfg=SMALL, kv_bf16=True, B=6, P=8, n_ops=60, seeds=(1, 2), bar=BF16_LOGIT_TOL, graph=False,
                      shared=False, manager=None,
                      # a bf16 pool refuses shared attention and tree verification (paged_infer.h)
                      kinds=tuple(k for k in FULL_KINDS if k not in ("set_shared", "verify_tree"))),
    "evict": dict(cfg=SMALL, kv_bf16=False, B=4, P=16, n_ops=60, seeds=(1, 2), bar=LOGIT_TOL, graph=False,
                  shared=False, manager=12, kinds=("admit", "ragged", "step_host", "step_dev", "fork", "release")),
    "chain6": dict(cfg=CHAIN, kv_bf16=False, B=6, P=16, n_ops=50, seeds=(1, 2), bar=LOGIT_TOL, graph=True,
                   shared=False, manager=None, kinds=FULL_KINDS),
}


def capacity(profile):
    """pages of the profile's manager: the engine's own holds B x maxT / P"""
    p = PROFILES[profile]
    return p["manager"] if isinstance(p["manager"], int) else p["B"] * (p["cfg"]["maxT"] // p["P"])


class _CachedRef64(ref64.Ref64):
    """Ref64 with its float64 weight views kept: the decoder calls them once per fed chunk and layer"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._cache = {}
        self.wte64 = self.wte.astype(np.float64)
        self.lnf = (self._t(14).astype(np.float64), self._t(15).astype(np.float64))

    def _mat(self, i, l, shape):
        key = (i, l)
        if key not in self._cache:
            self._cache[key] = super()._mat(i, l, shape)
        return self._cache[key]

    def logits(self, x):
        return ref64.ln(x, *self.lnf) @ self.wte64.T


def make_ref(cfgd, params, kv_bf16=False):
    return _CachedRef64(cfgd, params, kv_bf16=kv_bf16)


# ---------------------------------------------------------------- the decoder
class Decoder64:
    """one sequence, fed incrementally: float64 K/V of every layer (the rounded
    rows under kv_bf16, and the exact ones beside them for the K/V checker)"""

    def __init__(self, ref):
        self.ref = ref
        T, C, L = ref.cfg["maxT"], ref.C, ref.L
        self.K = np.zeros((L, T, C))
        self.V = np.zeros((L, T, C))
        self.Kx = np.zeros((L, T, C)) if ref.kv_bf16 else self.K
        self.Vx = np.zeros((L, T, C)) if ref.kv_bf16 else self.V
        self.n = 0

    def feed(self, tokens, ctx_shift=0):
        """appends the tokens at positions n ..; returns their float64 logits rows (len(tokens), V).
        ctx_shift (the sensitivity study of tests/test_engine_model.py only): the rows attend ctx_shift more
        keys than they should: -1 a context short by one key, +1 one stale key past the end"""
        ref, n0, T = self.ref, self.n, len(tokens)
        assert T > 0 and n0 + T <= ref.cfg["maxT"], (n0, T)
        pos = np.arange(n0, n0 + T)
        x = ref.embed(np.asarray(tokens, np.int64), pos).astype(np.float64)
        for l in range(ref.L):
            self.K[l, n0:n0 + T], self.V[l, n0:n0 + T] = ref.kv_rows(x, l)
            if ref.kv_bf16:
                self.Kx[l, n0:n0 + T], self.Vx[l, n0:n0 + T] = ref.kv_rows_exact(x, l)
            x = ref.layer_out(x, l, [self.K[l]] * T, [self.V[l]] * T, pos + 1 + ctx_shift)
        self.n = n0 + T
        return ref.logits(x)

    def fork(self, n):
        assert 0 <= n <= self.n
        d = Decoder64(self.ref)
        for name in ("K", "V") + (("Kx", "Vx") if self.ref.kv_bf16 else ()):
            getattr(d, name)[:, :n] = getattr(self, name)[:, :n]
        d.n = n
        return d

    def rewind(self, n):
        assert 0 <= n <= self.n
        self.n = n


def forward64(ref, tokens):
    """the from-scratch pass: every row of one sequence"""
    return Decoder64(ref).feed(list(tokens))


def top2(row):
    """(argmax, margin to the runner-up) of a float64 row"""
    i = int(np.argmax(row))
    rest = np.delete(row, i)
    return i, float(row[i] - rest.max())


# ---------------------------------------------------------------- what an op must leave
class Expect:
    def __init__(self, kind):
        self.kind = kind
        self.touched = {}    # slot -> dict(lo, n, row, tie): rows [lo, lo + n) written and kept, the last one's row
        self.verify = None   # per slot None or (n_accepted, accepted draft tokens)
        self.fork = None     # (src, dst, n)
        self.full_fork = False
        self.fresh_needed = 0  # fresh pages the op takes when nothing is evicted
        self.free_before = 0   # free pages before the op
        self.private_before = []  # per slot: it held a page of its own before the op
        self.pos_before = []
        self.fed_before = []   # per slot: a pass had written its logits row before the op
        self.passed_before = False  # some pass had run on the engine before the op
        self.evicted = []      # the slots the op paged out
        self.cow = []          # (slot, page index) of every private copy the op took


class Obs:
    """what the engine reports after an op.  pos, next_ids [B]; logits [B][V] float32; kv[l][b] = (K, V) rows
    [0, pos[b]); free_pages; pages / refs (a caller's BlockManager: the page list of every slot and {page:
    holders}), plan (shared attention on: (units, unit_of [B], shared_tokens [B])), result: the call's own
    return (next ids of a pass, (n_accepted, tokens) lists of a verify)"""

    def __init__(self, pos, next_ids, logits, kv, free_pages, pages=None, refs=None, plan=None, result=None):
        self.pos = [int(p) for p in pos]
        self.next_ids = np.asarray(next_ids, np.int32).copy()
        self.logits = np.asarray(logits, np.float32)
        self.kv, self.free_pages, self.pages, self.refs, self.plan, self.result = kv, free_pages, pages, refs, plan, result


class CheckFailed(AssertionError):
    def __init__(self, check, slot, where, detail):
        self.check, self.slot = check, slot
        profile, seed, index = where
        super().__init__(f"check '{check}' failed: slot {slot}, profile {profile}, seed {seed}, op {index}: {detail}")


# ---------------------------------------------------------------- the model
class EngineModel:
    def __init__(self, profile, seed):
        p = PROFILES[profile]
        self.profile, self.seed = profile, seed
        self.cfg, self.B, self.P, self.bar, self.kv_bf16 = p["cfg"], p["B"], p["P"], p["bar"], p["kv_bf16"]
        self.maxT, self.V = self.cfg["maxT"], self.cfg["V"]
        self.params = synth.params(self.cfg, seed=seed)
        self.ref = make_ref(self.cfg, self.params, kv_bf16=self.kv_bf16)
        self.capacity = capacity(profile)
        self.evicting = profile == "evict"
        B = self.B
        self.hist = [[] for _ in range(B)]
        self.dec = [Decoder64(self.ref) for _ in range(B)]
        self.pend = [None] * B      # the pending id; None: invalid (fresh, released, rewound, a shorter fork)
        self.tie = [False] * B      # the pending id came from an exempt near-tie row
        self.row = [None] * B       # float64 logits of the last fed token; None where the engine's row is stale
        self.pages = [[] for _ in range(B)]
        self._page = 0
        self.graph, self.shared, self.verify_attn, self.splits = p["graph"], p["shared"], 0, 0
        self.picks = self.exempt = 0
        self.cow = []               # (slot, page index) of every private copy the current op took
        self.fed = [False] * B      # the slot's logits row has been written since the engine was made
        # the engine's registers as the model would report them (observe()): untouched by everything but a pick
        self.img_next = np.zeros(B, np.int32)
        self.img_logits = np.zeros((B, self.V), np.float32)

    # ---- queries
    def pos(self, b):
        return len(self.hist[b])

    def live(self, b):
        return self.pos(b) > 0

    def fresh(self, b):
        return self.pos(b) == 0 and not self.pages[b]

    def holders(self, page):
        return sum(page in pl for pl in self.pages)

    def free_pages(self):
        return self.capacity - len({pg for pl in self.pages for pg in pl})

    def block_table(self):
        bt = np.full((self.B, self.maxT // self.P), -1, np.int32)
        for b, pl in enumerate(self.pages):
            bt[b, :len(pl)] = pl
        return bt

    def greedy(self, b, k):
        """the float64 greedy continuation of slot b from its pending id: rows [r_0 .. r_m] (r_0 the pending
        id's) and ids [g_1 .. g_m], g_i = argmax r_{i-1}; cut (m < k) at the first row whose top-2 margin does
        not exceed 2 x bar, or at the end of the context.  Leaves the slot as it was."""
        d, n0 = self.dec[b], self.dec[b].n
        rows, ids, tok = [], [], self.pend[b]
        while True:
            rows.append(d.feed([tok])[0])
            tok, margin = top2(rows[-1])
            if len(ids) == k or margin <= 2 * self.bar or d.n >= self.maxT:
                break
            ids.append(tok)
        d.rewind(n0)
        return rows, ids

    def margin_after(self, b, tokens):
        """the float64 top-2 margin of the row slot b would hold after these tokens; leaves the slot as it was"""
        d, n0 = self.dec[b], self.dec[b].n
        row = d.feed(list(tokens))[-1]
        d.rewind(n0)
        return top2(row)[1]

    # ---- pages
    def _new_page(self):
        self._page += 1
        return self._page

    def _append_pages(self, pages, b, lo, n):
        """positions [lo, lo + n) of slot b: a page with another holder is replaced by a private copy, a
        missing one is taken fresh.  Works on `pages` (the model's lists or a copy); returns the fresh pages taken"""
        took = 0
        for i in range(lo // self.P, (lo + n - 1) // self.P + 1):
            if i < len(pages[b]):
                if sum(pages[b][i] in pl for pl in pages) > 1:
                    pages[b][i] = self._new_page()
                    took += 1
                    if pages is self.pages:
                        self.cow.append((b, i))
            else:
                assert i == len(pages[b]), (b, i, len(pages[b]))
                pages[b].append(self._new_page())
                took += 1
        return took

    def _page_effects(self, op, pages):
        """the page side of an op on `pages`; returns the fresh pages it takes"""
        k, took = op["kind"], 0
        if k in ("admit", "ragged"):
            for b, t in enumerate(op["seqs"]):
                if len(t):
                    took += self._append_pages(pages, b, self.pos(b), len(t))
        elif k in ("step_host", "step_dev"):
            for b in range(self.B):
                took += self._append_pages(pages, b, self.pos(b), 1)
        elif k == "verify":
            for b, d in enumerate(op["drafts"]):
                if d is not None:
                    took += self._append_pages(pages, b, self.pos(b), len(d) + 1)
        elif k == "verify_tree":
            for b, t in enumerate(op["trees"]):
                if t is not None:
                    took += self._append_pages(pages, b, self.pos(b), len(t[0]) + 1)
        elif k == "fork":
            n = self.pos(op["src"]) if op["n"] == -1 else op["n"]
            pages[op["dst"]] = pages[op["src"]][:n // self.P]
            if n % self.P:
                pages[op["dst"]].append(self._new_page())
                took += 1
        elif k == "release":
            pages[op["slot"]] = []
        elif k == "reset":
            for b in range(self.B):
                pages[b] = []
        elif k == "reserve":
            need = -(-op["ctx"] // self.P)
            for b in range(self.B):
                lo = self.pos(b) // self.P
                if need > lo:
                    took += self._append_pages(pages, b, lo * self.P, (need - lo) * self.P)
        return took

    def standin_evictions(self, op):
        """the evict profile without an engine: SOME eviction mask under which a step fits the pool (the slot
        with the most private pages goes first).  Not the engine's LRU choice, which the model never predicts:
        it only keeps the model's own runs inside the pool."""
        mask = [False] * self.B
        if not op["kind"].startswith("step"):
            return mask
        while True:
            pages = [[] if mask[b] else list(pl) for b, pl in enumerate(self.pages)]
            need = 0
            for b in range(self.B):
                need += self._append_pages(pages, b, 0 if mask[b] else self.pos(b), 1)
            if len({pg for pl in pages for pg in pl}) <= self.capacity:
                return mask
            private = [sum(sum(pg in q for q in pages) == 1 for pg in pl) if not mask[b] else -1
                       for b, pl in enumerate(pages)]
            mask[int(np.argmax(private))] = True

    # ---- picks
    def _pick(self, b, row):
        i, margin = top2(row)
        self.row[b], self.pend[b], self.tie[b] = row, i, margin <= 2 * self.bar
        self.picks += 1
        self.fed[b] = True
        self.exempt += self.tie[b]
        self.img_logits[b] = row.astype(np.float32)
        self.img_next[b] = int(np.argmax(self.img_logits[b]))

    def adopt(self, b, token):
        """an exempt row: the engine's id is the slot's pending id from here on"""
        assert self.tie[b]
        self.pend[b] = int(token)
        self.img_next[b] = int(token)

    def _drop(self, b):
        self.hist[b], self.dec[b], self.pend[b], self.row[b], self.tie[b] = [], Decoder64(self.ref), None, None, False

    def _touch(self, exp, b, lo, kept, row):
        d = self.dec[b]
        self._pick(b, row)
        exp.touched[b] = dict(lo=lo, n=kept, row=row, tie=self.tie[b],
                              ref=[(d.Kx[l, lo:lo + kept].copy(), d.Vx[l, lo:lo + kept].copy())
                                   for l in range(self.ref.L)])

    # ---- the ops
    def apply(self, op, evicted=None):
        """moves the model through `op` and returns what the engine must show.  evicted (the evict profile):
        the slots gpt2_decode_evicted reported for this op; they restart at position 0 before the op's tokens land"""
        k = op["kind"]
        assert k in PROFILES[self.profile]["kinds"], k
        exp = Expect(k)
        exp.free_before = self.free_pages()
        exp.private_before = [any(self.holders(pg) == 1 for pg in pl) for pl in self.pages]
        exp.pos_before = [self.pos(b) for b in range(self.B)]
        exp.fed_before = list(self.fed)
        exp.passed_before = any(self.fed)
        exp.fresh_needed = self._page_effects(op, [list(pl) for pl in self.pages])
        exp.evicted = [b for b in range(self.B) if evicted is not None and evicted[b]]
        pend0 = list(self.pend)  # a device-fed step feeds an evicted slot's old pending id at position 0
        for b in exp.evicted:
            self._drop(b)
            self.pages[b] = []
        self.cow = exp.cow = []
        self._page_effects(op, self.pages)
        if k in ("admit", "ragged"):
            for b, t in enumerate(op["seqs"]):
                if len(t):
                    lo = self.pos(b)
                    rows = self.dec[b].feed(list(t))
                    self.hist[b] += [int(x) for x in t]
                    self._touch(exp, b, lo, len(t), rows[-1])
        elif k in ("step_host", "step_dev"):
            for b in range(self.B):
                tok = op["tokens"][b] if k == "step_host" else pend0[b]
                assert tok is not None, f"slot {b} has no valid pending id"
                lo = self.pos(b)
                row = self.dec[b].feed([tok])[0]
                self.hist[b].append(int(tok))
                self._touch(exp, b, lo, 1, row)
        elif k in ("verify", "verify_tree"):
            exp.verify = [None] * self.B
            for b in range(self.B):
                arg = op["drafts"][b] if k == "verify" else op["trees"][b]
                if arg is None:
                    continue
                assert self.pend[b] is not None, f"slot {b} has no valid pending id"
                ids, parents = (list(arg), list(range(len(arg)))) if k == "verify" else (list(arg[0]), list(arg[1]))
                assert tr.valid(parents, ids) and len(ids) <= MR - 1
                lo, d = self.pos(b), self.dec[b]
                tok = [self.pend[b]] + ids
                top = [-1] * len(tok)  # the float64 greedy id of every node the walk reaches
                cur, row = 0, d.feed([tok[0]])[0]
                while True:
                    top[cur] = top2(row)[0]
                    kids = [c for c in range(cur + 1, len(tok)) if parents[c - 1] == cur and tok[c] == top[cur]]
                    if not kids:
                        break
                    cur = kids[0]
                    row = d.feed([tok[cur]])[0]
                path = tr.accept(tok, top, parents)
                assert (path[-1] if path else 0) == cur and d.n == lo + len(path) + 1
                self.hist[b] += [int(tok[0])] + [int(tok[c]) for c in path]
                exp.verify[b] = (len(path), [int(tok[c]) for c in path], path)
                self._touch(exp, b, lo, len(path) + 1, row)
        elif k == "fork":
            src, dst = op["src"], op["dst"]
            n = self.pos(src) if op["n"] == -1 else op["n"]
            assert 1 <= n <= self.pos(src) and src != dst
            self.hist[dst], self.dec[dst] = self.hist[src][:n], self.dec[src].fork(n)
            self.row[dst] = None
            exp.fork, exp.full_fork = (src, dst, n), n == self.pos(src)
            if exp.full_fork:
                self.pend[dst], self.tie[dst], self.img_next[dst] = self.pend[src], self.tie[src], self.img_next[src]
            else:
                self.pend[dst], self.tie[dst] = None, False
        elif k == "release":
            self._drop(op["slot"])
        elif k == "reset":
            for b in range(self.B):
                self._drop(b)
        elif k == "rewind":
            for b, n in enumerate(op["pos"]):
                if n != self.pos(b):
                    assert 0 < n < self.pos(b)
                    self.hist[b] = self.hist[b][:n]
                    self.dec[b].rewind(n)
                    self.pend[b], self.row[b], self.tie[b] = None, None, False
        elif k == "set_graph":
            self.graph = bool(op["on"])
        elif k == "set_shared":
            self.shared = bool(op["on"])
        elif k == "set_verify_attention":
            self.verify_attn = op["request"]
        elif k == "set_attn_splits":
            self.splits = op["splits"]
        else:
            assert k == "reserve", k
        return exp

    # ---- the model's own report
    def observe(self, exp=None, plan_fn=None):
        """an Obs of the model's own values: what an engine that is exactly right would report"""
        L = self.ref.L
        kv = [[(self.dec[b].K[l, :self.pos(b)].astype(np.float32), self.dec[b].V[l, :self.pos(b)].astype(np.float32))
               for b in range(self.B)] for l in range(L)]
        refs = {pg: self.holders(pg) for pl in self.pages for pg in pl}
        plan = None
        if self.shared:
            plan = (plan_fn or plan_units)(self.block_table(), [self.pos(b) for b in range(self.B)], self.P)
        result = None
        if exp is not None and exp.verify is not None:
            result = ([None if v is None else v[0] for v in exp.verify],
                      [None if v is None else v[1] + [int(self.img_next[b])] for b, v in enumerate(exp.verify)])
            if exp.kind == "verify_tree":
                result += ([None if v is None else list(v[2]) for v in exp.verify],)
        elif exp is not None and exp.touched:
            result = self.img_next.copy()
        return Obs([self.pos(b) for b in range(self.B)], self.img_next, self.img_logits.copy(), kv, self.free_pages(),
                   [list(pl) for pl in self.pages], refs, plan, result)


def plan_units(bt, pos, P, min_tiles=1, min_members=2):
    """the header's plan on page lists, as (units, unit_of [B], shared_tokens [B])"""
    import shared_ref64 as sr
    units, skip = sr.plan(np.asarray(bt), np.asarray(pos), P, min_tiles, min_members)
    unit_of = np.full(len(pos), -1, np.int32)
    for u, (m, _) in enumerate(units):
        unit_of[m] = u
    return len(units), unit_of, 64 * np.asarray(skip, np.int32)


# ---------------------------------------------------------------- the checker
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_op(model, exp, prev, obs, index=-1):
    """holds `obs` (after the op) to the model (already moved by apply) and to `prev` (the Obs before the op).
    Returns dict(logit = worst |engine - float64| / bar, kv = worst K/V ratio / KV_RTOL, exempt = exempt rows of
    this op).  Adopts the engine's id on exempt rows.  Raises CheckFailed naming the check and the slot."""
    where = (model.profile, model.seed, index)
    B, P, L = model.B, model.P, model.ref.L
    worst = dict(logit=0.0, kv=0.0, exempt=0)

    def fail(check, slot, detail):
        raise CheckFailed(check, slot, where, detail)

    # 1. positions
    for b in range(B):
        if obs.pos[b] != model.pos(b):
            fail("position", b, f"engine {obs.pos[b]}, model {model.pos(b)}")
    # 2. touched slots
    for b, t in exp.touched.items():
        own = int(np.argmax(obs.logits[b]))
        if int(obs.next_ids[b]) != own:
            fail("next-id-own-argmax", b, f"next id {int(obs.next_ids[b])}, first argmax of the engine's row {own}")
        if not t["tie"] and int(obs.next_ids[b]) != model.pend[b]:
            fail("next-id-float64", b, f"next id {int(obs.next_ids[b])}, float64 argmax {model.pend[b]} with a "
                                       f"margin above {2 * model.bar:.1e}")
        diff = float(np.abs(obs.logits[b].astype(np.float64) - t["row"]).max())
        worst["logit"] = max(worst["logit"], diff / model.bar)
        if not diff <= model.bar:
            fail("logits", b, f"|engine - float64| = {diff:.3e} > {model.bar:.1e}")
        if t["tie"]:
            worst["exempt"] += 1
            model.adopt(b, obs.next_ids[b])
    if exp.verify is not None:
        n_acc, toks = obs.result[:2]
        nodes = obs.result[2] if len(obs.result) > 2 else None  # a tree pass: the accepted drafts' node indices
        for b, v in enumerate(exp.verify):
            if v is None:
                if n_acc[b] is not None:
                    fail("verify-walk", b, f"untouched, n_accepted {n_acc[b]}")
                continue
            if n_acc[b] != v[0] or list(toks[b][:-1]) != v[1] or toks[b][-1] != int(obs.next_ids[b]) or \
                    (nodes is not None and list(nodes[b]) != list(v[2])):
                fail("verify-walk", b, f"engine accepted {n_acc[b]}: {toks[b]}; the model's walk {v[0]}: {v[1]} "
                                       f"then {model.pend[b]}")
    elif exp.touched and obs.result is not None:
        for b in exp.touched:
            if int(obs.result[b]) != int(obs.next_ids[b]):
                fail("next-id-own-argmax", b, f"the call returned {int(obs.result[b])}, the device holds "
                                              f"{int(obs.next_ids[b])}")
    # 3. untouched slots
    for b in range(B):
        if b in exp.touched:
            continue
        # the logits buffer's first content means nothing: the engine's FIRST pass writes every row, a never-fed
        # slot's from its (still empty) decode row.  From then on every untouched row is held bit for bit
        if (exp.fed_before[b] or exp.passed_before) and \
                not np.array_equal(_bits(obs.logits[b]), _bits(prev.logits[b])):
            fail("untouched", b, "logits row changed")
        want = prev.next_ids[exp.fork[0]] if exp.full_fork and b == exp.fork[1] else prev.next_ids[b]
        if int(obs.next_ids[b]) != int(want):
            fail("untouched", b, f"pending id {int(prev.next_ids[b])} -> {int(obs.next_ids[b])}")
        # (its position: check 1 holds every slot's, and the model moves none but the op's)
    # 4. K/V rows
    for b in range(B):
        n = min(prev.pos[b], obs.pos[b])
        if b in exp.evicted:
            continue
        for l in range(L):
            for w in (0, 1):
                if not np.array_equal(_bits(obs.kv[l][b][w][:n]), _bits(prev.kv[l][b][w][:n])):
                    rows = np.nonzero((_bits(obs.kv[l][b][w][:n]) != _bits(prev.kv[l][b][w][:n])).any(-1))[0]
                    fail("kv-prefix", b, f"layer {l} {'KV'[w]} rows {rows[:4].tolist()} of [0, {n}) changed")
    for b, t in exp.touched.items():
        lo = t["lo"]
        before = [[(prev.kv[l][b][0][:lo], prev.kv[l][b][1][:lo])] for l in range(L)] if b not in exp.evicted else \
            [[(np.zeros((0, model.ref.C), np.float32),) * 2] for l in range(L)]
        try:
            r = ref64.check_kv(before, [[obs.kv[l][b]] for l in range(L)], [lo], [t["n"]],
                               ref=[[t["ref"][l]] for l in range(L)], rtol=KV_RTOL[model.kv_bf16],
                               kv_bf16=model.kv_bf16)
        except ref64.KVMismatch as e:
            fail("kv-written", b, str(e))
        worst["kv"] = max(worst["kv"], r / KV_RTOL[model.kv_bf16])
    if exp.fork:
        src, dst, n = exp.fork
        for l in range(L):
            for w in (0, 1):
                if not np.array_equal(_bits(obs.kv[l][dst][w][:n]), _bits(obs.kv[l][src][w][:n])):
                    fail("fork-copy", dst, f"layer {l} {'KV'[w]}: the first {n} rows differ from slot {src}'s")
    # 5. pages
    if not model.evicting and obs.free_pages != model.free_pages():
        fail("free-pages", -1, f"engine {obs.free_pages}, model {model.free_pages()}")
    if obs.pages is not None:
        for b, t in exp.touched.items():
            for i in range(t["lo"] // P, (obs.pos[b] - 1) // P + 1):
                if obs.refs[obs.pages[b][i]] != 1:
                    fail("written-page-private", b, f"page index {i} (page {obs.pages[b][i]}) has "
                                                    f"{obs.refs[obs.pages[b][i]]} holders after a write")
        for b in range(B):
            if len(obs.pages[b]) != len(model.pages[b]):
                fail("page-sharing", b, f"{len(obs.pages[b])} pages, model {len(model.pages[b])}")
        for pg in {pg for pl in obs.pages for pg in pl}:
            held = sum(pg in pl for pl in obs.pages)
            if obs.refs[pg] != held:
                fail("page-sharing", -1, f"page {pg}: refs {obs.refs[pg]}, listed by {held} slots")
        for a in range(B):
            for b in range(a + 1, B):
                for i in range(min(len(obs.pages[a]), len(obs.pages[b]))):
                    if (obs.pages[a][i] == obs.pages[b][i]) != (model.pages[a][i] == model.pages[b][i]):
                        fail("page-sharing", b, f"page index {i} of slots {a} and {b}: engine "
                                                f"{obs.pages[a][i]} / {obs.pages[b][i]}, model "
                                                f"{model.pages[a][i]} / {model.pages[b][i]}")
        # evictions are not predicted: the free count is held to the engine's own lists there
        if model.evicting and obs.free_pages != model.capacity - len({pg for pl in obs.pages for pg in pl}):
            fail("free-pages", -1, f"engine {obs.free_pages} free, its lists hold "
                                   f"{len({pg for pl in obs.pages for pg in pl})} of {model.capacity}")
    if model.evicting and exp.evicted:
        if not exp.fresh_needed > exp.free_before:
            fail("eviction", exp.evicted[0], f"evicted although the op needed {exp.fresh_needed} fresh pages and "
                                             f"{exp.free_before} were free")
        # The LRU policy pages a sequence out for a page with ONE holder.  Before: the slot held such a page, or
        # gains one in this op (it writes: a fresh page or a private copy -- every slot of a step does, so in a
        # step this half always holds), or a co-holder of one of its pages leaves in this op.  After: every page
        # it shared is still where the other holders had it (their rows are held bit for bit by check 4).
        steps = exp.kind in ("step_host", "step_dev")
        for b in exp.evicted:
            mates = {c for c in range(B) if c != b and set(prev.pages[c]) & set(prev.pages[b])} \
                if prev.pages is not None else set()
            left = any(c in exp.evicted or any(s == c for s, _ in exp.cow) for c in mates)
            if exp.pos_before[b] and not (exp.private_before[b] or steps or b in exp.touched or left):
                fail("eviction", b, "evicted while every page it held was shared")
            if prev.pages is None or obs.pages is None:
                continue
            for i, pg in enumerate(prev.pages[b]):
                for c in mates - set(exp.evicted):
                    if i >= len(prev.pages[c]) or prev.pages[c][i] != pg:
                        continue
                    t = exp.touched.get(c)
                    if t is not None and t["lo"] // P <= i <= (obs.pos[c] - 1) // P:
                        continue  # c wrote there: the page, or a private copy of it
                    if i >= len(obs.pages[c]) or obs.pages[c][i] != pg:
                        fail("eviction", b, f"page {pg} (index {i}), shared with slot {c}, did not stay with it")
    # 6. shared attention
    if obs.plan is not None and obs.pages is not None:
        n_units, unit_of, tok = obs.plan
        for u in range(n_units):
            members = [b for b in range(B) if unit_of[b] == u]
            if len(members) < 2:
                fail("shared-plan", u, f"unit of {len(members)} members")
            t = int(tok[members[0]])
            if t <= 0 or t % 64:
                fail("shared-plan", members[0], f"{t} shared tokens")
            for m in members:
                if int(tok[m]) != t or t > obs.pos[m]:
                    fail("shared-plan", m, f"{int(tok[m])} shared tokens in a unit of {t}, position {obs.pos[m]}")
                head, own = obs.pages[members[0]][:-(-t // P)], obs.pages[m][:-(-t // P)]
                if len(own) < -(-t // P) or own != head:
                    fail("shared-plan", m, f"pages {own} differ from slot {members[0]}'s {head} under {t} tokens")
        for b in range(B):
            if unit_of[b] >= n_units or (unit_of[b] < 0 and tok[b] != 0):
                fail("shared-plan", b, f"unit {unit_of[b]} of {n_units}, {tok[b]} shared tokens")
    return worst


# ---------------------------------------------------------------- the generator
class Trace:
    """iterating yields ops; each is generated from the model's state when it is asked for, so the driver must
    have applied (and checked) the one before.  Op i does not depend on n_ops."""

    def __init__(self, profile, seed, n_ops=None):
        self.p = PROFILES[profile]
        self.model = EngineModel(profile, seed)
        self.n_ops = self.p["n_ops"] if n_ops is None else n_ops
        self.rng = np.random.default_rng([seed, zlib.crc32(profile.encode())])  # the profile's own stream
        self.i = 0
        self.kinds = self.p["kinds"]
        self._macro, self._deck, self._round = None, [], 0
        self._vmode = 0

    def __iter__(self):
        return self

    def __next__(self):
        while self.i < self.n_ops:
            if self._macro is None:
                self._macro = self._next_macro()
            try:
                op = next(self._macro)
            except StopIteration:
                self._macro = None
                continue
            if op is None or op["kind"] not in self.kinds:
                continue
            m = self.model
            if m.evicting and not op["kind"].startswith("step") and \
                    m._page_effects(op, [list(pl) for pl in m.pages]) > m.free_pages():
                continue  # evictions are left to the steps: a pass that pages out one of its own slots fails
            self.i += 1
            return op
        raise StopIteration

    # ---- helpers
    def toks(self, n):
        return [int(t) for t in self.rng.integers(0, self.model.V, n)]

    def _slots(self, pred):
        return [b for b in range(self.model.B) if pred(b)]

    def _pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))] if xs else None

    def _settle(self, b, toks):
        """host-chosen tokens end on a row the greedy check has power over: the last token is drawn again (up
        to 8 times) while the row it leaves is a near-tie (float64 top-2 margin within 2 x bar)"""
        m = self.model
        for _ in range(8):
            if m.margin_after(b, toks) > 2 * m.bar:
                break
            toks = toks[:-1] + self.toks(1)
        return toks

    def _step_host(self):
        m = self.model
        return dict(kind="step_host", tokens=[self._settle(b, self.toks(1))[0] for b in range(m.B)])

    def _step_dev(self):
        """a device-fed step, where every slot has a valid pending id, room, and at most one slot would land
        on a near-tie row"""
        m = self.model
        if not all(m.pend[b] is not None for b in range(m.B)) or not self._room_for_all(1):
            return None
        if sum(m.margin_after(b, [m.pend[b]]) <= 2 * m.bar for b in range(m.B)) > 1:
            return None
        return dict(kind="step_dev", tokens=None)

    def _ragged(self, want, tag):
        m = self.model
        seqs = [[] for _ in range(m.B)]
        for b, n in want.items():
            n = min(n, m.maxT - 8 - m.pos(b))
            if n > 0:
                head = [m.pend[b]] if m.pend[b] is not None and n == 2 else []
                seqs[b] = self._settle(b, head + self.toks(n - len(head)))
        if not any(seqs):
            return None
        return dict(kind=tag, seqs=seqs)

    def _admit(self, slots, lo=1, hi=70):
        m = self.model
        return self._ragged({b: int(self.rng.integers(lo, hi + 1)) for b in slots if m.pos(b) == 0}, "admit")

    def _room_for_all(self, n):
        m = self.model
        return all(m.pos(b) + n < m.maxT - 8 for b in range(m.B))

    def _housekeeping(self):
        """keeps every context short of the end: a slot past 3/4 of it is released"""
        m = self.model
        for b in range(m.B):
            if m.pos(b) > 3 * m.maxT // 4:
                yield dict(kind="release", slot=b)

    def _fill(self):
        """every slot live (an admission for those that are not)"""
        m = self.model
        dead = self._slots(lambda b: not m.live(b))
        if dead:
            yield self._admit(dead, 3, 40)

    def _validate(self):
        """every slot live with a valid pending id: one ragged token for those without"""
        m = self.model
        yield from self._fill()
        bad = self._slots(lambda b: m.pend[b] is None)
        if bad:
            yield self._ragged({b: 1 for b in bad}, "ragged")

    def _free_slot(self, keep=()):
        """a fresh slot for a fork: releases the shortest other slot when there is none"""
        m = self.model
        fresh = self._slots(lambda b: m.fresh(b) and b not in keep)
        if fresh:
            return fresh[0], None
        cands = sorted(self._slots(lambda b: b not in keep), key=lambda b: (m.pos(b), b))
        if not cands:
            return None, None
        return cands[0], dict(kind="release", slot=cands[0])

    # ---- macros
    def _m_admit(self):
        m = self.model
        fresh = self._slots(lambda b: m.pos(b) == 0)
        if fresh:
            yield self._admit(fresh[:max(1, len(fresh) // 2)])
        yield from self._m_mix()

    def _m_mix(self):
        """0, 1 and many tokens per slot in one call, an admission among them when a slot is free"""
        m = self.model
        want = {}
        for b in range(m.B):
            c = (b + self._round) % 3
            if c == 1:
                want[b] = 1
            elif c == 2:
                want[b] = int(self.rng.integers(2, 40)) if m.live(b) else int(self.rng.integers(1, 71))
        yield self._ragged(want, "ragged")

    def _m_steps(self):
        m = self.model
        yield from self._fill()
        if self._room_for_all(2):
            yield self._step_host()
            yield self._step_dev()

    def _draft(self, b, mode, n):
        """mode 0: wrong from index 0; 1: wrong from the middle; 2: all right; 3: no draft (a plain step)"""
        m = self.model
        n = min(n, m.maxT - 8 - m.pos(b) - 1)
        if n <= 0 or mode == 3:
            return []
        rows, ids = m.greedy(b, n)
        k = len(ids)
        wrong = lambda r: int(np.argmin(r))  # noqa: E731  far below the top of its row in both arithmetics
        if mode == 2 and k:
            return ids
        if mode == 1 and k:
            j = max(1, k // 2)
            return (ids[:j] + [wrong(rows[j])] + self.toks(n))[:max(n, j + 1)]
        return ([wrong(rows[0])] + self.toks(n))[:n]

    def _m_verify(self):
        m = self.model
        yield from self._validate()
        drafts = []
        for b in range(m.B):
            mode = (b + self._vmode) % 5
            if mode == 4 or m.pend[b] is None or m.pos(b) + MR >= m.maxT - 8:
                drafts.append(None)
            else:
                drafts.append(self._draft(b, mode, int(self.rng.integers(1, MR))))
        self._vmode += 1
        if any(d is not None for d in drafts):
            yield dict(kind="verify", drafts=drafts)
        yield self._step_dev()

    def _tree(self, b, shape):
        """the greedy path plus wrong siblings; shape 0: the path under the SECOND child of the root, a wrong
        branch with a child of its own before it; 1: wrong siblings only; 2: a chain with one wrong sibling at
        the end"""
        m = self.model
        rows, ids = m.greedy(b, 3)
        low = lambda r, i: int(np.argsort(r)[i])  # noqa: E731
        if shape == 1 or not ids:
            return [low(rows[0], 0), low(rows[0], 1)], [0, 0]
        if shape == 2:
            t, par = list(ids), list(range(len(ids)))
            return t + [low(rows[len(ids)], 0)], par + [len(ids)]
        t, par = [low(rows[0], 0), ids[0], low(rows[0], 1), self.toks(1)[0]], [0, 0, 0, 1]
        node = 2  # the node that carries ids[0]
        for d in range(1, len(ids)):
            t += [low(rows[d], 0), ids[d]]
            par += [node, node]
            node = len(t)
        return t[:MR - 1], par[:MR - 1]

    def _m_tree(self):
        m = self.model
        yield from self._validate()
        trees = []
        for b in range(m.B):
            c = (b + self._vmode) % 4
            if c == 3 or m.pend[b] is None or m.pos(b) + MR >= m.maxT - 8:
                trees.append(None)
            else:
                trees.append(self._tree(b, c))
        self._vmode += 1
        if any(t is not None for t in trees):
            yield dict(kind="verify_tree", trees=trees)

    def _src(self, need):
        """a live slot with at least `need` tokens: the longest one, grown first when it is shorter"""
        m = self.model
        src = max(range(m.B), key=lambda b: (m.pos(b), -b))
        return src, (self._ragged({src: need - m.pos(src)}, "ragged" if m.live(src) else "admit")
                     if m.pos(src) < need else None)

    def _m_fork_rewind(self):
        """fork all of a source, rewind the fork into a page it shares, append there"""
        m, P = self.model, self.model.P
        src, grow = self._src(2 * P + 3)
        yield grow
        dst, rel = self._free_slot(keep=(src,))
        yield rel
        if dst is None or not m.fresh(dst) or m.pos(src) < P + 2:
            return
        yield dict(kind="fork", src=src, dst=dst, n=-1)
        pos = [m.pos(b) for b in range(m.B)]
        pos[dst] = P + P // 2 if m.pos(dst) > 2 * P else P // 2
        if m.pos(src) // P >= 3:
            pos[src] = (m.pos(src) // P - 1) * P  # the source onto a page boundary, below the length it shares
        yield dict(kind="rewind", pos=pos)
        # the fork stays inside the shared page it was rewound into; the source opens the one at its boundary
        yield self._ragged({dst: P // 2 - 1, src: 1}, "ragged")

    def _m_verify_release_fork(self):
        """a verify pass leaves rejected rows in a slot's pages; the slot is released and a fork lands in it"""
        m, P = self.model, self.model.P
        yield from self._validate()
        live = self._slots(lambda b: m.pend[b] is not None and m.pos(b) + MR < m.maxT - 8)
        if len(live) < 2:
            return
        src = max(live, key=lambda b: (m.pos(b), -b))
        x = self._pick([b for b in live if b != src])
        drafts = [None] * m.B
        drafts[x] = self._draft(x, 0, MR - 1)
        drafts[src] = self._draft(src, 2, 3)
        yield dict(kind="verify", drafts=drafts)
        yield dict(kind="release", slot=x)
        n = m.pos(src) - 1
        if n % P == 0:
            n -= 1
        if n >= 1:
            yield dict(kind="fork", src=src, dst=x, n=n)
            yield self._ragged({x: 2}, "ragged")

    def _m_forks(self):
        """forks of every kind off one source: a multiple of the page size, all of it, a ragged shorter prefix"""
        m, P = self.model, self.model.P
        src, grow = self._src(max(2 * P + 5, 72 if m.shared or self.p["shared"] else 0))
        yield grow
        for which in range(3):
            n = [(m.pos(src) // P) * P if m.pos(src) % P else m.pos(src) - P, -1, m.pos(src) - P // 2 - 1][which]
            if n != -1 and (n < 1 or n >= m.pos(src)):
                continue
            dst, rel = self._free_slot(keep=(src,) + tuple(self._slots(lambda b: b != src and m.pages[b][:1] ==
                                                                   m.pages[src][:1] and m.live(b))))
            yield rel
            if dst is not None and m.fresh(dst):
                yield dict(kind="fork", src=src, dst=dst, n=n)
        if self._room_for_all(1):
            yield from self._fill()
            yield self._step_host()

    def _m_dissolve(self):
        """a member of a shared prefix is rewound below it (or released): a unit shrinks or dissolves"""
        m, P = self.model, self.model.P
        shared = self._slots(lambda b: m.pages[b] and m.holders(m.pages[b][0]) > 1)
        if len(shared) < 2:
            return
        pos = [m.pos(b) for b in range(m.B)]
        b = shared[-1]
        if pos[b] > P:
            pos[b] = P  # onto a page boundary, below the shared length
            yield dict(kind="rewind", pos=pos)
        else:
            yield dict(kind="release", slot=b)
        if self._room_for_all(1):
            yield from self._fill()
            yield self._step_host()
        for c in shared[:-1][1:]:
            yield dict(kind="release", slot=c)
            break

    def _m_release_fork(self):
        """the evict profile: a release makes the room a fork's tail page needs"""
        m, P = self.model, self.model.P
        live = sorted(self._slots(m.live), key=lambda b: (-m.pos(b), b))
        if len(live) < 2:
            return
        src, x = live[0], live[-1]
        yield dict(kind="release", slot=x)
        n = m.pos(src) - 1 if self._round % 2 else (m.pos(src) // P) * P
        if 1 <= n <= m.pos(src):
            yield dict(kind="fork", src=src, dst=x, n=n)
        yield from self._m_steps()

    def _m_reserve(self):
        m = self.model
        ctx = min(m.maxT, (max(m.pos(b) for b in range(m.B)) // m.P + 2) * m.P)
        yield dict(kind="reserve", ctx=ctx)
        yield from self._m_steps()

    def _m_reset(self):
        yield dict(kind="reset")
        yield self._admit(list(range(self.model.B))[::2])

    def _toggle(self, op, then, step=False):
        """a toggle, then a pass at once: the macro's own first op, or (step) a decode step before a macro that
        starts with something else"""
        yield op
        if step:
            yield from self._fill()
            if self._room_for_all(1):
                yield self._step_host()
        yield from then()

    def _next_macro(self):
        if not self._deck:
            self._round += 1
            m, first = self.model, self._round == 1
            T = self._toggle
            if self.model.evicting:
                deck = [self._m_mix, self._m_steps, self._m_release_fork, self._m_admit, self._m_steps, self._m_forks]
            else:
                deck = [
                    lambda: T(dict(kind="set_graph", on=not m.graph), self._m_steps),
                    lambda: T(dict(kind="set_verify_attention", request=1), self._m_verify),
                    self._m_fork_rewind,
                    lambda: T(dict(kind="set_verify_attention", request=2), self._m_verify_release_fork),
                    lambda: T(dict(kind="set_attn_splits", splits=2), self._m_reserve, step=True),
                    lambda: T(dict(kind="set_shared", on=not m.shared), self._m_forks, step=True),
                    lambda: T(dict(kind="set_verify_attention", request=0),
                              self._m_tree if "verify_tree" in self.kinds else self._m_verify),
                    self._m_dissolve,
                    lambda: T(dict(kind="set_graph", on=not m.graph), self._m_mix),
                    lambda: T(dict(kind="set_shared", on=not m.shared), self._m_forks, step=True),
                    self._m_dissolve,
                    lambda: T(dict(kind="set_attn_splits", splits=0), self._m_verify),
                ]
                if "set_shared" not in self.kinds:
                    deck = [d for i, d in enumerate(deck) if i != 9]
                order = self.rng.permutation(len(deck))
                deck = [deck[i] for i in order]
                if first:
                    deck.insert(len(deck) // 2, self._m_reset)
            self._deck = ([self._m_admit] if first else []) + deck

        macro = self._deck.pop(0)

        def run():
            yield from self._housekeeping()
            yield from macro()
        return run()


def make_trace(profile, seed, n_ops=None):
    return Trace(profile, seed, n_ops)
