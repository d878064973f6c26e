"""hpa_paged_attention_verify_tree (the verify kernel with an ancestor mask,
hpa_verify.hip) against the float64 reference of tests/attn_ref64.py on each
row's visible key set, gathered: the cached context below start plus the
node's own ancestors.  Pools are attn_ref64.poisoned_pool's: every byte
outside the contexts is 0xFF.

Six sequences (fp32 pools of page size 8, 16, 32, 64; waves 0 / 4 / 8):
    start    0: 8 nodes -- node 0 on an empty cache
    start    5: 1 node
    start   60: 8 nodes -- slots 60..67 straddle the 64-token tile edge, with
                ancestors on both sides of it
    start 1000: len = 0 -- skipped, its output row keeps the fill
    start  250: 8 nodes
    start 1016: 8 nodes -- the last slot is key 1023
under four tree shapes (tree_ref64.SHAPES): a star, two chains of 3 off the
root (7 nodes), a binary tree, a chain.

The slots of a sequence's nodes all hold finite K and V (a hidden sibling's V
row is multiplied by a weight of exactly 0, which needs a finite value), and
node i's V is U(-1, 1) -+ 40 (1 + i // 2): far from every other node's.  In
every row one head is "hot_hidden" where the row has a hidden node: the query
is aimed (attn_ref64._aimed) at that node's key, so a leak of the hidden key
would put nearly all the weight on a V row at least 40 away.
test_a_leak_would_show asserts on the CPU, in float64, that making the sibling
visible moves the output by more than 100 x the row's unit (the smallest such
move is 7.1e4 units).  The other head cycles through the row's own key, its
parent's, the last cached key, key 0 and a uniform query.

The pass rule is the project's: every output finite and ratio <= BAR
(tests/test_attn_ref64.py).  With chain masks the output bits equal
hpa_paged_attention_verify's on the same inputs."""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
import tree_ref64 as tr
from test_attn_ref64 import BAR

pytestmark = pytest.mark.gpu

PAGES = (8, 16, 32, 64)
STARTS = (0, 5, 60, 1000, 250, 1016)
FULL = (8, 1, 8, 0, 8, 8)       # nodes per sequence; the two-chains shape has 7 where these have 8
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_U8 = ctypes.POINTER(ctypes.c_ubyte)
HS, NH, C = ar.HS, ar.NH, ar.C
_cases, _sets = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _cases.clear()
    _sets.clear()


class _TreeCases:
    """K, V per sequence (start + nodes rows; a len = 0 sequence still owns one
    row's context), one query row per node, each row's visible keys, the
    float64 reference on them and the same with the aimed-at hidden key added"""

    def __init__(self, shape):
        self.shape = shape
        par_full = tr.SHAPES[shape]
        self.seqs, self.q, self.vis, self.kind, self.hid = [], [], [], [], []
        self.lens = np.array([min(n, len(par_full) + 1) for n in FULL], np.int32)
        self.starts = np.array(STARTS, np.int32)
        self.row0 = np.concatenate([[0], np.cumsum(np.maximum(self.lens, 1))[:-1]]).astype(np.int32)
        self.anc = []
        self.seq = []
        for b, (st, n) in enumerate(zip(STARTS, self.lens)):
            rng = np.random.default_rng([7, b, st, len(par_full)])
            m = st + max(n, 1)
            K = rng.uniform(-1, 1, (m, C)).astype(np.float32)
            V = rng.uniform(-1, 1, (m, C)).astype(np.float32)
            for i in range(n):  # node i's V far from every other node's
                V[st + i] += np.float32(40.0 if i % 2 else -40.0) * (1 + i // 2)
            self.seqs.append((K, V))
            par = par_full[:max(n, 1) - 1]
            masks, see = tr.anc_masks(par), tr.visible(par)
            for r in range(max(n, 1)):
                vis = np.concatenate([np.arange(st), st + np.nonzero(see[r])[0]]).astype(np.int64)
                hidden = [i for i in range(n) if not see[r][i]]
                q = np.zeros(C, np.float32)
                kinds, hid = [], [-1, -1]
                for h in range(NH):
                    c = slice(h * HS, (h + 1) * HS)
                    if hidden and h == (r + b) % NH:
                        # prefer a hidden node below r (inside the row's tile bound), else one above it
                        low = [i for i in hidden if i < r]
                        j = st + (low[(r + b) % len(low)] if low else hidden[0])
                        kind, hid[h] = "hot_hidden", j
                    else:
                        kind = ("hot_own", "hot_parent", "uniform", "hot_cached", "hot_key0")[(r + 2 * b + h) % 5]
                        if kind == "hot_parent" and r == 0:
                            kind = "hot_own"
                        if kind in ("hot_cached", "hot_key0") and st == 0:
                            kind = "hot_own"
                        j = {"hot_own": st + r, "hot_parent": st + (par[r - 1] if r else 0), "hot_cached": st - 1,
                             "hot_key0": 0, "uniform": -1}[kind]
                    q[c] = rng.uniform(-2, 2, HS) if kind == "uniform" else ar._aimed(K[vis, c], K[j, c])
                    kinds.append(kind)
                self.q.append(q)
                self.vis.append(vis)
                self.kind.append(kinds)
                self.hid.append(hid)
                self.anc.append(masks[r] if n else 0)
                self.seq.append(b)
        self.q = np.stack(self.q)
        self.anc = np.array(self.anc, np.uint8)
        self.R = len(self.q)
        self.live = np.array([self.lens[b] > 0 for b in self.seq])
        self.out, self.unit = np.zeros((self.R, C)), np.ones((self.R, C))
        self.leak = np.full((self.R, NH), np.nan)  # |out with the hidden key visible - out| / unit, worst dim
        for i in range(self.R):
            if not self.live[i]:
                continue
            K, V = self.seqs[self.seq[i]]
            for h in range(NH):
                c = slice(h * HS, (h + 1) * HS)
                ref = ar.attend(self.q[i, c], K[self.vis[i], c], V[self.vis[i], c])
                self.out[i, c], self.unit[i, c] = ref.out[0], ref.unit[0]
                if self.hid[i][h] >= 0:
                    more = np.concatenate([self.vis[i], [self.hid[i][h]]])
                    leaked = ar.attend(self.q[i, c], K[more, c], V[more, c])
                    self.leak[i, h] = (np.abs(leaked.out[0] - ref.out[0]) / ref.unit[0]).max()

    def ratios(self, got):
        got = np.asarray(got, np.float64)
        with np.errstate(invalid="ignore"):
            r = (np.abs(got - self.out) / self.unit).reshape(-1, NH, HS).max(2)
        return np.where(np.isfinite(got).reshape(-1, NH, HS).all(2), r, np.inf)


def _tree_cases(shape):
    if shape not in _cases:
        _cases[shape] = _TreeCases(shape)
    return _cases[shape]


class _Set:
    """a shape's cases in a poisoned pool of page size P, tables uploaded;
    pool_kw: attn_ref64.poisoned_pool's further arguments (tests/test_gpu_pool_large.py)"""

    def __init__(self, hip, shape, P, dtype=ar.HPA_F32, **pool_kw):
        self.cs = cs = _tree_cases(shape)
        self.Rp = (cs.R + 15) // 16 * 16
        self.pool, tables = ar.poisoned_pool(hip, cs, P, dtype, **pool_kw)
        self.tables = tables
        self.maxp = tables.shape[1]
        self.d_q = hip.DeviceBuffer.from_array(cs.q)
        self.d_bt = hip.DeviceBuffer.from_array(np.ascontiguousarray(tables))
        self.d_start = hip.DeviceBuffer.from_array(cs.starts)
        self.d_row0 = hip.DeviceBuffer.from_array(cs.row0)
        self.d_len = hip.DeviceBuffer.from_array(cs.lens)
        self.d_anc = hip.DeviceBuffer.from_array(np.concatenate([cs.anc, np.zeros(self.Rp - cs.R, np.uint8)]))
        self.d_out = hip.DeviceBuffer(self.Rp * C * 4)

    def launch(self, hip, T=None, chain_kernel=False, pool=None):
        """one launch into the 0xFF-filled output; returns (rc, rows (R, C), raw bits)"""
        L = hip.lib()
        hip.check(L.hpa_memset_async(self.d_out.ptr, 0xFF, self.d_out.nbytes))
        c = ctypes.cast
        T = int(self.cs.lens.max()) if T is None else T
        pool = ctypes.addressof(self.pool.s) if pool is None else pool
        head = (c(self.d_q.ptr, _F), pool, 0, c(self.d_bt.ptr, _I), self.maxp, c(self.d_start.ptr, _I),
                c(self.d_row0.ptr, _I), c(self.d_len.ptr, _I))
        if chain_kernel:
            rc = L.hpa_paged_attention_verify(*head, len(self.cs.lens), T, c(self.d_out.ptr, _F))
        else:
            rc = L.hpa_paged_attention_verify_tree(*head, c(self.d_anc.ptr, _U8), len(self.cs.lens), T,
                                                   c(self.d_out.ptr, _F))
        hip.check(L.hpa_synchronize())
        raw = self.d_out.download(self.Rp * C)
        return rc, hip.from_frag(raw, self.cs.R, C), raw.view(np.uint32).copy()


def _set(hip, shape, P):
    if (shape, P) not in _sets:
        _sets[shape, P] = _Set(hip, shape, P)
    return _sets[shape, P]


@pytest.mark.parametrize("shape", list(tr.SHAPES))
def test_a_leak_would_show(shape):
    """CPU, float64: for every hot_hidden (row, head) the output with the
    aimed-at sibling made visible differs from the reference by more than
    100 x the row's unit; every shape but the chain has such rows"""
    cs = _tree_cases(shape)
    leak = cs.leak[~np.isnan(cs.leak)]
    if shape == "chain":  # a chain hides only the nodes after a row: still hidden keys, past the row's own
        assert leak.size > 0
    else:
        own = [cs.starts[cs.seq[i]] + i - cs.row0[cs.seq[i]] for i in range(cs.R)]  # each row's own slot
        below = sum(1 for i in range(cs.R) for h in range(NH) if 0 <= cs.hid[i][h] < own[i])
        assert below >= 8, below  # hidden nodes in slots below the row's own, inside its tile bound
    assert leak.size >= 12 and leak.min() > 100.0, (leak.size, leak.min())
    print(f"TREEATTN {shape}: {leak.size} hot_hidden (row, head)s, smallest leak {leak.min():.3e} units")


@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("shape", list(tr.SHAPES))
def test_tree_against_float64(hip, shape, P):
    """every row of the five live sequences within the bar on its visible
    keys, at 0 / 4 / 8 waves, each launch twice bit for bit; the len = 0
    sequence's row and the padding rows keep their fill.

    Measured worst ratios on the MI355X (the TREEATTN lines this test prints),
    over every shape, page size and wave count, against the bar of 40.8:
    hot_hidden 1.653, uniform 0.953, hot_own 0.072, hot_parent 0.072,
    hot_key0 0.016, hot_cached 0.014"""
    s = _set(hip, shape, P)
    cs = s.cs
    L = hip.lib()
    try:
        for waves in (0, 4, 8):
            hip.check(L.hpa_set_attention_waves(waves))
            rc, got, bits = s.launch(hip)
            assert rc == 0
            r = cs.ratios(got)[cs.live]
            kinds = np.array(cs.kind)[cs.live]
            by = {k: float(r[kinds == k].max()) for k in sorted(set(kinds.ravel()))}
            print(f"TREEATTN {shape} P={P} waves={waves} rows={int(cs.live.sum())} worst={r.max():.3f} "
                  + " ".join(f"{k}={v:.3f}" for k, v in by.items()))
            assert np.isfinite(got[cs.live]).all()
            i, h = np.unravel_index(np.argmax(r), r.shape)
            assert r.max() <= BAR, f"waves {waves} live row {i} head {h} ({kinds[i][h]}): ratio {r.max():.2f} > {BAR}"
            assert (got[~cs.live].view(np.uint32) == 0xFFFFFFFF).all(), "a len = 0 sequence's output row was written"
            pad = hip.from_frag(bits.view(np.float32), s.Rp, C)[cs.R:]
            assert (pad.view(np.uint32) == 0xFFFFFFFF).all()
            rc2, _, bits2 = s.launch(hip)
            assert rc2 == 0 and np.array_equal(bits, bits2), "two launches on the same inputs differ"
    finally:
        hip.check(L.hpa_set_attention_waves(0))


@pytest.mark.parametrize("P", PAGES)
def test_chain_masks_give_the_chain_kernels_bits(hip, P):
    """the chain shape's masks are the causal mask of a chain pass: bit for
    bit hpa_paged_attention_verify's output on the same inputs"""
    s = _set(hip, "chain", P)
    assert s.cs.anc[s.cs.live].tolist() == [(2 << (i - s.cs.row0[b])) - 1 for i, b in enumerate(s.cs.seq) if s.cs.live[i]]
    L = hip.lib()
    try:
        for waves in (0, 4, 8):
            hip.check(L.hpa_set_attention_waves(waves))
            rc_t, _, tree_bits = s.launch(hip)
            rc_c, _, chain_bits = s.launch(hip, chain_kernel=True)
            assert rc_t == 0 and rc_c == 0
            assert np.array_equal(tree_bits, chain_bits), waves
    finally:
        hip.check(L.hpa_set_attention_waves(0))


def test_tree_refuses_nine_rows_and_other_pools(hip):
    """T = 9, T = 0, a bf16 pool and a pool of head size 128: nonzero, nothing
    launched (the output keeps its fill)"""
    s = _set(hip, "star", 16)
    for T in (9, 0):
        rc, _, bits = s.launch(hip, T=T)
        assert rc != 0 and (bits == 0xFFFFFFFF).all(), T
    for field, value in (("dtype", ar.HPA_BF16), ("head_size", 128)):
        fake = type(s.pool.s)()
        ctypes.memmove(ctypes.addressof(fake), ctypes.addressof(s.pool.s), ctypes.sizeof(fake))
        setattr(fake, field, value)  # refused on the struct's fields, before anything is launched
        rc, _, bits = s.launch(hip, pool=ctypes.addressof(fake))
        assert rc != 0 and (bits == 0xFFFFFFFF).all(), field
    o = _Set(hip, "star", 16, ar.HPA_BF16)  # a real bf16 pool too
    rc, _, bits = o.launch(hip)
    assert rc != 0 and (bits == 0xFFFFFFFF).all()
