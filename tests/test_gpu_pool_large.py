"""Every kernel that turns (page, head, slot, d) into an address, on page pools
of more than 2, 4 and 8 GiB per layer: the cases, references and bars of the
small-pool modules, with only the page indices moved.

Stand-alone kernels (one-layer pools, NH = 2, one pool alive at a time):

    pool   bytes per layer    marks inside (offset from the layer's base)
    fp32   8 GiB + 64 MiB     2^31 B, 2^32 B, 2^33 B (= 2^31 elements)
    bf16   8 GiB + 64 MiB     2^31 B, 2^32 B (= 2^31 elements), 2^33 B (= 2^32 elements)
    fp8    4 GiB + 64 MiB     2^31 B (= 2^31 elements), 2^32 B (= 2^32 elements)

at the dtype's smallest page size (8, 8, 16) and at P = 64.  A mark is where a
32-bit byte offset or element index would wrap (tests/pool_marks.py, whose
32-bit models tests/test_pool_index_host.py holds against the library at
these very pages).  The sequences' pages are the pool's first pages, the pages
below and from each mark upward and the pool's last pages -- the same number
at each of them, nearest first (pool_marks.candidates) -- handed out in a
random permutation (attn_ref64.poisoned_pool), so every longer sequence's
block table jumps across all marks.  The slab is 0xFF everywhere else: a
wrapped address reads NaN, or another sequence's page under a hot key, and
fails by an O(1) margin.  Every test asserts from its tables that each mark
has pages in use on both sides and that page 0 and the last page are in use,
and prints them (POOLLARGE lines).

Bars: BAR of tests/test_attn_ref64.py for attention, the float64 bound of
tests/test_gpu_fused.py for the fused QKV append, bit equality for copies,
moves and fills -- nothing new is measured or tuned.

The engine (two layers of 4 GiB + 64 MiB each, so layer 1's base lies past
2^32 bytes; C = 768: a page is 1536 P elem_bytes bytes, so a mark falls inside
a page and inside one head's tile): the layer harnesses of
tests/test_gpu_layer_hard.py and tests/test_gpu_kv_append.py with an engine
opener that makes the first-fit allocator hand out the pages of the zones
around the marks (big_opener), and one placement-invariance script.

A test skips only when hpa_pool_create itself reports that the allocation
failed; the message carries the size.

Measured on the MI355X (profiles/EXPERIMENTS.md has the whole table): worst
attention ratios 5.548 (fp32 decode), 4.973 (bf16 decode), 5.919 (fp8
prefill), 3.256 (verify), 1.653 (verify_tree) against BAR = 40.8 -- the
small-pool figures to the printed digit; the fused append at 0.017 of its
bound; engine layer outputs 3.5e-07 .. 1.30e-06 (fp32 weights) and 6.4e-04
(bf16 weights) against 1e-5 / 5.0e-6 / 4e-3; the module's 54 tests take 11 s.
"""
import ctypes

import numpy as np
import pytest

import attn_ref64 as ar
import pool_marks as pm
import test_gpu_attention_hard as tah
import test_gpu_attention_verify as tav
import test_gpu_attention_verify_tree as tat
import test_gpu_fused as tgf
import tree_ref64 as tr

pytestmark = pytest.mark.gpu

NH, HS, C = ar.NH, ar.HS, ar.C
POOLS = [(d, P) for d in (ar.HPA_F32, ar.HPA_BF16, ar.HPA_FP8) for P in (pm.MIN_PAGE[d], 64)]
F32_POOLS = [p for p in POOLS if p[0] == ar.HPA_F32]
_I = ctypes.POINTER(ctypes.c_int)
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _cases.clear()
    tat._cases.clear()


def _pool_id(p):
    return tah._pool_id(p)


def _geometry(dtype, P):
    """(pages, bytes per page, marks) of the big one-layer pool of (dtype, P)"""
    pb = pm.page_elems(NH, P) * pm.ELEM_BYTES[dtype]
    n = pm.BIG_LAYER_BYTES[dtype] // pb
    return n, pb, pm.marks(n * pb, pm.ELEM_BYTES[dtype])


POOL_FAILED = "page pool allocation failed"  # hpa_pool_create's message, and no other allocation's


def _skip_pool_failure(e, nbytes):
    if POOL_FAILED in str(e):
        pytest.skip(f"hpa_pool_create: the allocation of {nbytes} bytes ({nbytes / pm.GiB:.2f} GiB) failed")


class _SkippingPools:
    """the pagedattn module with a Pool that skips the test when hpa_pool_create
    reports that its allocation failed; every other failure is raised as it is"""

    def __init__(self, hip):
        self._hip = hip

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def Pool(self, *a, **kw):
        try:
            return self._hip.Pool(*a, **kw)
        except RuntimeError as e:
            s = pm.ELEM_BYTES[int(kw.get("dtype", ar.HPA_F32))] * a[0] * a[3] * pm.page_elems(a[1], a[2])
            _skip_pool_failure(e, s)
            raise


def _decode_init(hip, m, nbytes, *a, **kw):
    """decode_init whose pool is created inside the engine: the library's last
    error is first set to another message by a call it refuses (3 attention
    waves; nothing is launched), so the pool's message after a failure is this
    call's and not an older one's"""
    assert hip.lib().hpa_set_attention_waves(3) != 0
    try:
        m.decode_init(*a, **kw)
    except RuntimeError as e:
        _skip_pool_failure(e, nbytes)
        raise


def _big_kw(dtype, P, need):
    n, pb, mk = _geometry(dtype, P)
    return dict(num_pages=n, candidates=pm.candidates(n, pb, mk, need))


def _assert_spread(what, dtype, P, tables, jump=True):
    """from the tables themselves: page 0, the last page, and both sides of every mark in use;
    jump: some sequence's own pages lie on both sides of every mark"""
    n, pb, mk = _geometry(dtype, P)
    used = np.unique(tables[tables >= 0])
    assert used[0] == 0 and used[-1] == n - 1, (what, used[0], used[-1], n)
    for m, (lo, hi) in pm.sides(used, pb, mk).items():
        up = -(-m // pb)
        assert lo >= 1 and hi >= 1 and up - 1 in used and up in used, (what, m, lo, hi)
    off = [row[row >= 0].astype(np.int64) * pb for row in tables]  # 64-bit: these offsets pass 2^31
    jumps = sum(all((o < m).any() and (o >= m).any() for m in mk) for o in off)
    assert jumps >= 1 or not jump, what
    print(f"POOLLARGE {what} {_pool_id((dtype, P))} pool={n * pb / pm.GiB:.3f}GiB pages={n} used={used.size} "
          f"tables_across_every_mark={jumps}/{len(tables)} | {pm.describe(used, pb, mk)}")


class _installed:
    """a big-pool set put where a small-pool module looks its sets up (that
    module's test functions then run on it unchanged), taken out again and
    its pool freed on exit"""

    def __init__(self, cache, key, make):
        self.cache, self.key, self.make = cache, key, make

    def __enter__(self):
        self.old = self.cache.pop(self.key, None)
        self.cache[self.key] = self.set = self.make()
        return self.set

    def __exit__(self, *exc):
        self.cache.pop(self.key, None)
        if self.old is not None:
            self.cache[self.key] = self.old
        self.set.pool.destroy()


def _cached(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


# ---------------------------------------------------------------- attention
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_decode_attention(hip, pool):
    """hpa_paged_attention_decode, _decode_frag, _decode_split and _decode_split_w over
    attn_ref64.decode_cases with the launches of LAUNCHES, as tests/test_gpu_attention_hard.py runs them"""
    dtype, P = pool
    cs = _cached(("d", dtype, P), lambda: ar.decode_cases(P, dtype))
    kw = _big_kw(dtype, P, ar.pages_needed(cs, P))
    make = lambda: tah._Set(_SkippingPools(hip), cs, P, dtype, **kw)
    with _installed(tah._sets, ("d", dtype, P), make) as s:
        assert s.pool.s.bytes == pm.BIG_LAYER_BYTES[dtype] > 4 * pm.GiB
        _assert_spread("decode", dtype, P, s.tables)
        for frag in (False, True):
            tah.test_decode(hip, pool, frag)
        for by_arg in (False, True):
            tah.test_decode_split(hip, pool, by_arg)


@pytest.mark.parametrize("ragged", [False, True], ids=["prefill", "prefill_ragged"])
@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_prefill_attention(hip, pool, ragged):
    dtype, P = pool
    cs = _cached(("p", dtype, ragged), lambda: ar.prefill_cases(dtype, lens=tah.RAGGED_LENS if ragged else (130,) * 4,
                                                               seed=2 if ragged else 1))
    kw = _big_kw(dtype, P, ar.pages_needed(cs, P))
    make = lambda: tah._Set(_SkippingPools(hip), cs, P, dtype, **kw)
    with _installed(tah._sets, ("p", dtype, P, ragged), make) as s:
        _assert_spread("prefill_ragged" if ragged else "prefill", dtype, P, s.tables)
        tah.test_prefill(hip, pool, ragged)


@pytest.mark.parametrize("pool", F32_POOLS, ids=_pool_id)
def test_verify_attention(hip, pool):
    """hpa_paged_attention_verify: both case batches of tests/test_gpu_attention_verify.py"""
    dtype, P = pool
    for name, (starts, lens) in (("main", (tav.STARTS, tav.LENS)), ("edge", (tav.EDGE_STARTS, tav.EDGE_LENS))):
        make = lambda: tav._Set(_SkippingPools(hip), starts, lens, P, dtype,
                                pool_kw=lambda cs: _big_kw(dtype, P, ar.pages_needed(cs, P)))
        with _installed(tav._sets, (name, P, dtype), make) as s:
            _assert_spread(f"verify_{name}", dtype, P, s.tables)
            if name == "main":
                tav.test_verify_against_float64(hip, P)
            else:
                tav.test_verify_skips_a_len0_sequence_and_straddles_the_tile_edge(hip, P)


@pytest.mark.parametrize("shape", list(tr.SHAPES))
@pytest.mark.parametrize("pool", F32_POOLS, ids=_pool_id)
def test_verify_tree_attention(hip, pool, shape):
    """hpa_paged_attention_verify_tree: the cases of tests/test_gpu_attention_verify_tree.py"""
    dtype, P = pool
    cs = tat._tree_cases(shape)
    kw = _big_kw(dtype, P, ar.pages_needed(cs, P))
    make = lambda: tat._Set(_SkippingPools(hip), shape, P, dtype, **kw)
    with _installed(tat._sets, (shape, P), make) as s:
        _assert_spread(f"verify_tree_{shape}", dtype, P, s.tables)
        tat.test_tree_against_float64(hip, shape, P)
        if shape == "chain":
            tat.test_chain_masks_give_the_chain_kernels_bits(hip, P)


# ---------------------------------------------------------------- copies, moves, fills
def _poisoned(hip, dtype, P, layers=1):
    n, pb, mk = _geometry(dtype, P)
    pool = _SkippingPools(hip).Pool(layers, NH, P, n, dtype=dtype)
    L = hip.lib()
    hip.check(L.hpa_memset_async(pool.s.base, 0xFF, pool.s.bytes), "poison")
    hip.check(L.hpa_synchronize())
    return pool, n, pb, mk


def _page_bytes(hip, pool, page, pb):
    out = np.empty(pb, np.uint8)
    hip.check(hip.lib().hpa_memcpy(out.ctypes.data, hip.lib().hpa_pool_tile(pool.ref, 0, int(page), 0, 0), pb), "page read")
    return out


@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_copy_pages_across_every_mark(hip, pool):
    """hpa_pool_copy_pages, one launch: per mark a pair below -> above and a
    pair above -> below, and the pool's two ends (page 1 -> the last page, the
    last but one -> page 0).  Every destination byte-exact in every tile, the
    sources and every neighbouring page untouched (still 0xFF)."""
    dtype, P = pool
    big, n, pb, mk = _poisoned(hip, dtype, P)
    try:
        rng = np.random.default_rng([11, int(dtype), P])
        pairs = [(1, n - 1), (n - 2, 0)]
        for m in mk:
            up = m // pb
            assert up * pb == m  # page-aligned at NH = 2
            pairs += [(up - 1, up), (up + 2, up - 3)]
        src = {s: rng.integers(0, 255, pb, dtype=np.uint8) for s, _ in pairs}  # never 0xFF: no byte looks untouched
        for s, data in src.items():
            hip.check(hip.lib().hpa_memcpy(hip.lib().hpa_pool_tile(big.ref, 0, s, 0, 0), data.ctypes.data, pb), "page write")
        big.copy_pages([s for s, _ in pairs], [d for _, d in pairs])
        hip.check(hip.lib().hpa_synchronize())
        want = dict(src)
        want.update({d: src[s] for s, d in pairs})
        near = sorted({q for s, d in pairs for p in (s, d) for q in range(p - 2, p + 3) if 0 <= q < n})
        for q in near:
            got = _page_bytes(hip, big, q, pb)
            if q in want:
                assert np.array_equal(got, want[q]), (q, int(np.flatnonzero(got != want[q])[0]))
            else:
                assert (got == 0xFF).all(), (q, int(np.flatnonzero(got != 0xFF)[0]))
        print(f"POOLLARGE copy_pages {_pool_id(pool)} pool={n * pb / pm.GiB:.3f}GiB pairs (src, dst) {pairs} "
              f"marks at pages {[m // pb for m in mk]}: byte-exact, {len(near) - len(want)} neighbouring pages untouched")
    finally:
        big.destroy()


@pytest.mark.parametrize("pool", F32_POOLS, ids=_pool_id)
def test_compact_path_across_every_mark(hip, pool):
    """hpa_pool_compact_path on paths whose source and destination slots lie in
    pages on opposite sides of a mark, against the numpy move of
    tests/tree_ref64.py (compact_in_place) on the sequences' slot rows; rows
    outside the moved slots and the neighbouring pages keep their bits"""
    dtype, P = pool
    big, n, pb, mk = _poisoned(hip, dtype, P)
    try:
        rng = np.random.default_rng([13, P])
        paths = [(P - 3, [3, 5, 7]), (2 * P - 2, [2, 4]), (P - 3, [1, 4, 5, 6, 7]), (P - 2, [7])]
        # two sequences per zone, their logical pages alternating sides: the pool's two ends, then each mark
        tables, cases = [[0, n - 1, 1, n - 2], [n - 3, 2, n - 4, 3]], paths[:2]
        for zi, m in enumerate(mk, 1):
            up = m // pb
            tables += [[up - 1, up, up - 2, up + 1], [up + 2, up - 3, up + 3, up - 4]]
            cases += [paths[(2 * zi) % 4], paths[(2 * zi + 1) % 4]]
        bt = np.array(tables, np.int32)
        B, ntok = len(bt), 4 * P
        rows = []
        for b in range(B):
            k = rng.uniform(-1, 1, (ntok, C)).astype(np.float32)
            v = rng.uniform(-1, 1, (ntok, C)).astype(np.float32)
            big.write_tokens(0, bt[b], k, v)
            rows.append((k, v))
        start = np.array([c[0] for c in cases], np.int32)
        acc = np.array([len(c[1]) for c in cases], np.int32)
        path = np.full((B, tr.MR), 99, np.int32)
        crossing = np.zeros(B, int)  # per sequence: moves whose source and destination pages lie on opposite sides
        for b, (st, p) in enumerate(cases):
            path[b, :len(p)] = p
            for k, src in enumerate(p, 1):
                sp, dp = int(bt[b, (st + src) // P]), int(bt[b, (st + k) // P])
                crossing[b] += sp != dp and (b < 2 or (sp * pb < mk[b // 2 - 1]) != (dp * pb < mk[b // 2 - 1]))
        assert crossing.min() >= 1, crossing
        d = [hip.DeviceBuffer.from_array(a) for a in (bt, start, path, acc)]
        hip.check(hip.lib().hpa_pool_compact_path(big.ref, ctypes.cast(d[0].ptr, _I), 4, ctypes.cast(d[1].ptr, _I),
                                                  ctypes.cast(d[2].ptr, _I), ctypes.cast(d[3].ptr, _I), B), "compact_path")
        hip.check(hip.lib().hpa_synchronize())
        for b, (st, p) in enumerate(cases):
            gk, gv = big.read_tokens(0, bt[b], ntok)
            for got, old in ((gk, rows[b][0]), (gv, rows[b][1])):
                want = old.copy()
                want[st:st + tr.MR] = tr.compact_in_place(old[st:st + tr.MR], p)
                assert not np.array_equal(want, old)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), b
        used = set(bt.ravel().tolist())
        near = sorted({q for p in used for q in (p - 1, p + 1) if 0 <= q < n and q not in used})
        for q in near:
            assert (_page_bytes(hip, big, q, pb) == 0xFF).all(), q
        print(f"POOLLARGE compact_path {_pool_id(pool)} pool={n * pb / pm.GiB:.3f}GiB tables {bt.tolist()} "
              f"moves across a mark or the pool's ends: {crossing.tolist()}; bit-exact, {len(near)} neighbouring pages untouched")
    finally:
        big.destroy()


@pytest.mark.parametrize("pool", POOLS, ids=_pool_id)
def test_fill_random_rows_do_not_depend_on_the_page(hip, pool):
    """hpa_pool_fill_random: the rows of (seed, sequence, position) on pages
    around every mark equal, bit for bit, the rows the same call leaves on a
    small pool; the slots past the context keep their 0xFF"""
    dtype, P = pool
    B, ctx, seed = 5, 2 * P + 3, 1234
    npg = (ctx + P - 1) // P
    small = hip.Pool(1, NH, P, B * npg, dtype=dtype)
    L = hip.lib()
    hip.check(L.hpa_memset_async(small.s.base, 0xFF, small.s.bytes), "poison")
    bt_small = np.arange(B * npg, dtype=np.int32).reshape(B, npg)
    big, n, pb, mk = _poisoned(hip, dtype, P)
    try:
        cand = pm.candidates(n, pb, mk, B * npg)[:B * npg]
        bt_big = np.random.default_rng([17, int(dtype)]).permutation(cand).astype(np.int32).reshape(B, npg)
        _assert_spread("fill_random", dtype, P, bt_big, jump=False)
        got = []
        for pool_, bt in ((small, bt_small), (big, bt_big)):
            if dtype == ar.HPA_FP8:
                pool_.set_scales(ar.K_SCALE[None, :], ar.V_SCALE[None, :])
            d_bt = hip.DeviceBuffer.from_array(bt)
            hip.check(L.hpa_pool_fill_random(pool_.ref, d_bt.ptr, npg, B, ctx, seed), "fill_random")
            hip.check(L.hpa_synchronize())
            got.append([pool_.read_tokens(0, bt[b], npg * P) for b in range(B)])
        for b in range(B):
            for wi in range(2):
                a, c = got[0][b][wi].view(np.uint32), got[1][b][wi].view(np.uint32)
                assert np.isfinite(got[1][b][wi][:ctx]).all() and np.isnan(got[1][b][wi][ctx:]).all(), (b, wi)
                assert np.array_equal(a, c), (b, "KV"[wi], int(np.argwhere(a != c)[0][0]))
        assert len({got[1][b][0][:ctx].tobytes() for b in range(B)}) == B  # the sequences' rows differ
    finally:
        big.destroy()
        small.destroy()


# ---------------------------------------------------------------- the fused QKV append
def _qkv_tables(n, pb, mk, P, pages_per):
    """one sequence per zone pair, its logical pages alternating between the
    two sides of a mark (or the pool's two ends)"""
    t = [[(k // 2) if k % 2 == 0 else n - 1 - k // 2 for k in range(pages_per)]]
    for m in mk:
        up = m // pb
        t.append([up - 1 - k // 2 if k % 2 == 0 else up + k // 2 for k in range(pages_per)])
        t.append([up + 8 + k // 2 if k % 2 == 0 else up - 9 - k // 2 for k in range(pages_per)])
    return np.array(t, np.int32)


def _check_append(hip, big, bt, seq_of_row, pos, acc, bound, pb, n):
    """appended K/V rows within the bound; every other slot of the sequences'
    pages and the pages next to them still 0xFF"""
    ntok = bt.shape[1] * big.s.page_size
    worst = 0.0
    for b in range(len(bt)):
        k, v = big.read_tokens(0, bt[b], ntok)
        mine = np.flatnonzero(seq_of_row == b)
        written = np.zeros(ntok, bool)
        written[pos[mine]] = True
        for got, lo in ((k, C), (v, 2 * C)):
            assert (got[~written].view(np.uint32) == 0xFFFFFFFF).all(), b
            for r in mine:
                err = np.abs(got[pos[r]] - acc[r, lo:lo + C])
                assert np.all(err <= bound[r, lo:lo + C]), (b, r)
                worst = max(worst, float((err / bound[r, lo:lo + C]).max()))
    used = set(bt.ravel().tolist())
    near = sorted({q for p in used for q in (p - 1, p + 1) if 0 <= q < n and q not in used})
    for q in near:
        assert (_page_bytes(hip, big, q, pb) == 0xFF).all(), q
    return worst, len(near)


@pytest.mark.parametrize("row_seq", [False, True], ids=["row_per_sequence", "row_seq"])
@pytest.mark.parametrize("pool", F32_POOLS, ids=_pool_id)
def test_fused_qkv_appends_either_side_of_every_mark(hip, pool, row_seq):
    """hpa_gemm_fused with the QKV epilogue through test_gpu_fused._run: one row
    per sequence, or (row_seq) runs of rows at consecutive positions that cross
    a page edge -- and with it a mark.  q and the appended K/V within that
    module's float64 bound; everything around them still poison."""
    dtype, P = pool
    big, n, pb, mk = _poisoned(hip, dtype, P)
    try:
        bt = _qkv_tables(n, pb, mk, P, 4)
        S = len(bt)
        _assert_spread("fused_qkv", dtype, P, bt, jump=False)
        rng = np.random.default_rng([19, P, int(row_seq)])
        if row_seq:  # 6 rows per sequence: from P - 3 (logical pages 0 | 1: the pages either side of the mark,
            # or page 0 and the last page) or from 2P - 2 (pages 1 | 2: one further away on each side)
            start = np.array([P - 3 if b % 2 or b == 0 else 2 * P - 2 for b in range(S)])
            seq = np.repeat(np.arange(S), 6).astype(np.int32)
            pos = np.concatenate([s + np.arange(6) for s in start]).astype(np.int32)
            args = (big, bt, pos, seq)
        else:  # logical page 1 of every sequence: the last page, then the first page above / a page below each mark
            seq = np.arange(S, dtype=np.int32)
            pos = np.array([2 * P - 1] + [P + (3 * b + (b % 2) * (P - 1)) % P for b in range(1, S)], np.int32)
            args = (big, bt, pos)
        M = len(pos)
        pages = bt[seq, pos // P].astype(np.int64)
        for j, m in enumerate(mk):  # the two sequences of a mark append on both of its sides
            mine = pages[(seq == 2 * j + 1) | (seq == 2 * j + 2)]
            assert (mine * pb < m).any() and (mine == m // pb).any(), (m, mine)
            assert not row_seq or (mine == m // pb - 1).any(), (m, mine)
        assert (pages == n - 1).any()
        out, acc, bound, keep = tgf._run(hip, hip.HPA_FEPI_QKV, M, C, 3 * C, 8, ln=True, rng=rng, pool_args=args)
        q = out.download((M, C))
        qr = float((np.abs(q - acc[:, :C]) / bound[:, :C]).max())
        assert np.all(np.abs(q - acc[:, :C]) <= bound[:, :C])
        worst, near = _check_append(hip, big, bt, seq, pos, acc, bound, pb, n)
        print(f"POOLLARGE fused_qkv {'row_seq' if row_seq else 'rows'} {_pool_id(pool)} rows={M} pages appended to "
              f"{sorted(set(pages.tolist()))} worst |err|/bound: q {qr:.3f} K/V {worst:.3f}; {near} neighbouring pages untouched")
    finally:
        big.destroy()


# ---------------------------------------------------------------- the engine on a big pool
import ref64  # noqa: E402
import synth  # noqa: E402
import test_gpu_kv_append as tka  # noqa: E402
import test_gpu_layer_hard as tlh  # noqa: E402

ENGINE_L = 2          # layer 1's base is itself past 2^32 bytes
SPARE_PAGES = 4096    # pages one spare prompt may hold


def plan_placement(slots, B, P, page_bytes, elem_bytes, max_ctx, fill_pages, appended):
    """Which of the manager's pages stay free for a batch, from the engine's
    page map alone (slots[i]: the pool slot of manager page i).

    The zones (pool_marks.candidates: the pool's start, either side of every
    mark, the pool's end) hold exactly the B * max_pages slots the batch can
    need.  The engine's fill takes the free pages lowest manager index first,
    sequence by sequence (sequence b's logical page lp is the (b fill_pages +
    lp)-th free page; a page a step has to open is the next free one, steps
    and then sequences in order), and the map scatters them over the zones.
    For an appended row to land in the pool's last page, the lowest-indexed
    zone pages are withheld (they stay with a spare prompt) until the last
    page's rank among the free ones is that of a page a step appends to
    (`appended`: (step, sequence, logical page)).  Returns (free manager pages,
    withheld manager pages, marks).

    What this relies on in the engine (a change there breaks the placement
    asserts of _Placement.check, loudly, not the addressing checks):
    block_manager.c bm_first_free (lowest free index first);
    paged_infer.c gpt2_decode_fill_random_ex (resets, then requests sequence by
    sequence), dec_ensure_pages / dec_grow (a step opens pages in sequence
    order) and page_map_create (a fixed permutation in groups of 1 or 16 pages
    with the tail left in place -- why pool_marks.engine_pages rounds to 16)."""
    N = len(slots)
    mk = pm.marks(N * page_bytes, elem_bytes)
    max_pages = -(-max_ctx // P)
    need = B * max_pages
    zone_slots = pm.candidates(N, page_bytes, mk, need)[:need]
    inv = np.empty(N, np.int64)
    inv[slots] = np.arange(N)
    zone = np.sort(inv[zone_slots])
    last = int(inv[N - 1])
    r = int(np.searchsorted(zone, last))
    grown = []
    for _, b, lp in sorted(appended):
        if lp >= fill_pages and (b, lp) not in grown:
            grown.append((b, lp))
    targets = sorted({b * fill_pages + lp for _, b, lp in appended if lp < fill_pages}
                     | {B * fill_pages + i for i in range(len(grown))})
    k = max(t for t in targets if t <= r)  # rank 0 is sequence 0's first page: position 0 is appended to
    withheld, free = zone[:r - k], zone[r - k:]
    assert B * fill_pages + len(grown) <= len(free), ("the batch would run out of pages", r, k, len(free))
    return free, withheld, mk


class _Placement:
    """what a big-pool engine was given and, once it closes, where its sequences' pages lay"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.pages = None  # [b]: pool slots of sequence b's pages, read as the engine closes

    def check(self, what, pos, steps):
        """from bm.pages(b), through the engine's page map"""
        pb, mk, N, P = self.page_bytes, self.marks, self.num_pages, self.P
        assert self.layer_bytes >= 1 << 32 and self.pages is not None
        rows_at = lambda b, t: int(self.pages[b][t // P])  # noqa: E731
        both = {m: [b for b in range(self.B)
                    if any((p + 1) * pb <= m for p in self.pages[b]) and any(p * pb >= m for p in self.pages[b])]
                for m in mk}
        for m in mk:
            assert both[m], (what, m)  # a sequence with rows stored below the mark and rows stored above it
        app = sorted({rows_at(b, int(pos[b]) + s) for b in range(self.B) for s in range(steps)})
        assert any(p * pb >= mk[-1] for p in app), (what, app)
        assert N - 1 in app, (what, app)
        allp = np.concatenate([np.asarray(p, np.int64) for p in self.pages])
        zone = set(pm.candidates(N, pb, mk, self.need)[:self.need].tolist())
        assert set(allp.tolist()) <= zone and len(set(allp.tolist())) == allp.size
        straddle = [int(m // pb) for m in mk if m % pb]
        print(f"POOLLARGE engine {what} layer={self.layer_bytes / pm.GiB:.3f}GiB x{ENGINE_L} pages={N} "
              f"page={pb}B batch_pages={allp.size} withheld={self.withheld} sequences_on_both_sides="
              f"{ {int(np.log2(m)): len(v) for m, v in both.items()} } appended_pages={app} "
              f"pages_holding_a_mark={straddle} in_use={[p in set(allp.tolist()) for p in straddle]} | "
              f"{pm.describe(allp, pb, mk)}")


def open_big(hip, cfgd, params, B, P, kv_dtype, w_dtype, max_ctx, fill_pages, appended):
    """an engine over a caller's BlockManager sized for ENGINE_LAYER_BYTES per
    layer: spare prompts (ids >= B) take every page, then the one that holds
    the planned zone pages lets go of them, so the first-fit allocator can only
    hand out zone pages.  Returns (model, placement); the model records its
    sequences' pages when it closes."""
    NH, C = cfgd["NH"], cfgd["C"]
    eb = pm.ELEM_BYTES[int(kv_dtype)]
    pb = pm.page_elems(NH, P) * eb
    N = pm.engine_pages(pb)
    keepers = -(-N // SPARE_PAGES)
    bm = hip.BlockManager(C, B + 2 + keepers, N, P, SPARE_PAGES)
    place = _Placement(B=B, P=P, page_bytes=pb, num_pages=N, layer_bytes=N * pb, need=B * -(-max_ctx // P))

    class BigModel(hip.Model):
        def close(self):
            if self.h and place.pages is None:
                place.pages = [place.slots[np.asarray(bm.pages(b), np.int64)].tolist() for b in range(B)]
            super().close()
            bm.close()

    m = BigModel(cfgd, params=params)
    m.set_manager(bm)
    _decode_init(hip, m, ENGINE_L * N * pb, B, P, max_ctx, kv_dtype=kv_dtype, w_dtype=w_dtype)
    place.slots = m.page_slots(N).astype(np.int64)
    assert np.array_equal(np.sort(place.slots), np.arange(N))
    free, withheld, place.marks = plan_placement(place.slots, B, P, pb, eb, max_ctx, fill_pages, appended)
    place.withheld = len(withheld)
    owner = np.full(N, -1, np.int64)            # spare prompt of every page: B the zone pages that will be freed,
    owner[free], owner[withheld] = B, B + 1     # B + 1 the withheld ones, then the keepers
    rest = np.flatnonzero(owner < 0)
    owner[rest] = B + 2 + np.arange(rest.size) // SPARE_PAGES
    L = hip.lib()
    for i, p in enumerate(owner.tolist()):      # first fit: page i goes to the i-th request
        blk = L.request_block(bm.h, p)
        assert blk and (i % 4096 or L.bm_block_index(bm.h, blk) == i), i
    assert bm.free_pages() == 0
    bm.free_prompt(B)
    assert bm.free_pages() == len(free) and sorted(bm.pages(B + 1)) == withheld.tolist()
    return m, place


def _appended(B, P, F, steps):
    pos = ref64.ragged_positions(B, P, F)
    return pos, sorted({(s, b, (int(pos[b]) + s) // P) for b in range(B) for s in range(steps)})


ENGINE_B = 20  # two row blocks; satisfies ref64.check_position_mix


@pytest.mark.parametrize("C,NH,P,kv,select,form", [
    pytest.param(768, 12, 16, "f32", 0, 0, id="five_launches-f32-P16"),
    pytest.param(768, 12, 16, "f32", 5, 3, id="chain6-f32-P16"),
    pytest.param(768, 12, 16, "fp8", 5, 3, id="chain6-fp8-P16"),
    pytest.param(128, 2, 16, "f32", 3, 2, id="chain_4wave-f32-P16"),
])
def test_engine_layer_peaked(hip, C, NH, P, kv, select, form):
    """tests/test_gpu_layer_hard.py's case, bars and all, on the big pool"""
    B = ENGINE_B
    pos, appended = _appended(B, P, tlh.F, 2)
    got = {}

    def opener(hip, C, NH, B, P, kv_dtype):
        cfgd = dict(maxT=tlh.MAX_CTX, V=1000, L=ENGINE_L, NH=NH, C=C)
        params = ar.peaked_params(cfgd, seed=900 + NH)
        m, got["place"] = open_big(hip, cfgd, params, B, P, kv_dtype, hip.HPA_F32, tlh.MAX_CTX, -(-tlh.F // P), appended)
        return cfgd, params, m

    tlh._run_case(hip, C, NH, B, P, kv, select, form, opener=opener)
    got["place"].check(f"layer_hard req{select} C={C} P={P} {kv}", pos, 2)


@pytest.mark.parametrize("C,NH,P,kv_bf16,w_bf16,select,form", [
    pytest.param(768, 12, 8, True, False, 5, 3, id="chain6-bf16-P8"),
    pytest.param(1024, 16, 32, True, False, 6, 3, id="chain8-bf16-P32"),
    pytest.param(768, 12, 8, True, True, None, 4, id="bf16_weight_chain-bf16-P8"),
])
def test_engine_kv_append(hip, C, NH, P, kv_bf16, w_bf16, select, form):
    """tests/test_gpu_kv_append.py's case, bars and all, on the big pool"""
    B = ENGINE_B
    pos, appended = _appended(B, P, tka.F, 4)
    got = {}

    def opener(hip, C, NH, B, P, kv_bf16, w_bf16, select, form):
        cfgd = dict(maxT=tka.MAX_CTX, V=1000, L=ENGINE_L, NH=NH, C=C)
        params = synth.params(cfgd, seed=700 + NH)
        m, got["place"] = open_big(hip, cfgd, params, B, P, hip.HPA_BF16 if kv_bf16 else hip.HPA_F32,
                                   hip.HPA_BF16 if w_bf16 else hip.HPA_F32, tka.MAX_CTX, -(-tka.F // P), appended)
        if select is not None:
            m.set_layer_kernel(select)
        assert m.layer_form() == form, (m.layer_form(), form)
        return cfgd, params, m

    tka._run_case(hip, C, NH, B, P, kv_bf16, w_bf16, select, form, opener=opener)
    got["place"].check(f"kv_append form{form} C={C} P={P} kv_bf16={int(kv_bf16)} w_bf16={int(w_bf16)}", pos, 4)


# ---------------------------------------------------------------- placement invariance of the serving paths
INV = dict(C=768, NH=12, B=4, P=16, MAX_CTX=256, V=1000, LENS=(5, 70, 130))


def plan_staged(slots, page_bytes, need, first_pages):
    """For the serving script, from the engine's page map: the zone pages in
    three stages.  Stage 1 (free before the prefill): first_pages pages whose
    highest manager index -- the last page the prefill hands out, the 130-token
    sequence's tail -- is the pool slot that holds the 2^32 B mark.  Stage 2
    (free before the fork, alone): the slot that holds the 2^31 B mark, which
    the fork's copied tail page then has to be.  Stage 3: the rest.

    Relies on block_manager.c bm_first_free (lowest free index first), on
    paged_infer.c's ragged prefill growing its sequences in order (dec_grow per
    sequence, so the 130-token one gets the highest of the stage-1 pages last)
    and on gpt2_decode_fork taking one fresh page for the partly filled tail;
    the asserts on seen["before_fork"] and pages[3] say so when that changes."""
    N = len(slots)
    mk = pm.marks(N * page_bytes, 4)
    zone_slots = pm.candidates(N, page_bytes, mk, need)[:need]
    inv = np.empty(N, np.int64)
    inv[slots] = np.arange(N)
    hold31, hold32 = int(mk[0] // page_bytes), int(mk[1] // page_bytes)
    assert mk[0] % page_bytes and mk[1] % page_bytes and {hold31, hold32} <= set(zone_slots.tolist())
    zone = np.sort(inv[zone_slots])
    src, dst = int(inv[hold32]), int(inv[hold31])
    lower = zone[(zone < src) & (zone != dst)]
    assert lower.size >= first_pages - 1, "too few zone pages below the 2^32 B page in the manager's order"
    # spread over the zones: every (lower.size // (first_pages - 1))-th of them
    stage1 = np.concatenate([lower[::max(1, lower.size // (first_pages - 1))][:first_pages - 1], [src]])
    stage3 = np.setdiff1d(zone, np.concatenate([stage1, [dst]]))
    return np.sort(stage1), dst, stage3, mk, (hold31, hold32)


def _inv_tokens():
    rng = np.random.default_rng(41)
    V = INV["V"]
    return dict(prompts=[rng.integers(0, V, n).astype(np.int32) for n in INV["LENS"]],
                scored=rng.integers(0, V, 9).astype(np.int32), readmit=rng.integers(0, V, 20).astype(np.int32))


def _next_ids(hip, m):
    out = np.zeros(m.B, np.int32)
    hip.check(hip.lib().hpa_memcpy(out.ctypes.data, m.next_ptr(), out.nbytes), "next ids")
    return out


def _serve(hip, m, tok, stream=None, stage=lambda name: None, greedy_steps=0):
    """the script; returns everything it computed.  stream: per sequence the
    greedy ids that follow its pending id after the fork (None: find them with
    greedy_steps plain steps and return)"""
    B, L = m.B, m.cfg.num_layers
    out = {}
    m.set_graph(True)
    stage("prefill")
    out["prefill_next"] = m.prefill_ragged(tok["prompts"] + [[]])[:3]
    out["prefill_logits"] = m.logits()[:3]
    lp, top, nxt = m.score([tok["scored"], [], [], []])
    out["score"] = (lp[0], top[0], nxt[:1])
    stage("fork")
    m.fork(2, 3)
    stage("rest")
    assert m.positions().tolist() == [14, 70, 130, 130]
    out["fork_kv"] = [m.read_kv(l, 3, 130) for l in range(L)]
    for l in range(L):
        for wi in range(2):
            assert np.array_equal(out["fork_kv"][l][wi].view(np.uint32), m.read_kv(l, 2, 130)[wi].view(np.uint32)), (l, wi)
    if stream is None:
        ids = [_next_ids(hip, m)] + [m.step(None) for _ in range(greedy_steps)]
        return np.stack(ids, 1)  # (B, 1 + greedy_steps): the pending id, then the greedy stream
    assert np.array_equal(_next_ids(hip, m), stream[:, 0])
    at = np.zeros(B, int)  # how far along its stream each sequence is

    def true(b, n):
        return stream[b, at[b] + 1:at[b] + 1 + n].tolist()

    def wrong(t):
        return int((t + 1) % INV["V"])

    out["verify"] = []
    for rnd in range(3):  # drafts: all true / a wrong id in the middle / none (a plain step) / sequence left out
        drafts = []
        for b in range(B):
            kind = (b + rnd) % 4
            d = true(b, 3 + rnd)
            if kind == 1:
                d[1] = wrong(d[1])
            drafts.append(d if kind < 2 else [] if kind == 2 else None)
        acc, toks, lps = m.verify(drafts, want_logprobs=True)
        out["verify"].append((acc, toks, [None if x is None else x.copy() for x in lps], m.positions()))
        for b in range(B):
            if acc[b] is not None:
                at[b] += acc[b] + 1
    trees = []
    for b in range(B):  # two branches off the pending id: a wrong chain first, the true chain second
        t = true(b, 3)
        trees.append(None if b == 1 else ([wrong(t[0]), wrong(t[1]), t[0], t[1], t[2], wrong(t[2])], [0, 1, 0, 3, 4, 4]))
    acc, toks, nodes = m.verify_tree(trees)
    out["tree"] = (acc, toks, nodes, m.positions())
    out["tree_logits"] = m.logits()[[0, 2, 3]]
    m.release(1)
    out["readmit_next"] = m.prefill_ragged([[], tok["readmit"], [], []])[1:2]
    out["steps"] = []
    m.set_logprobs(True)
    for _ in range(6):
        nxt = m.step(None)
        out["steps"].append((nxt, m.logprobs(), m.logits()))
    m.status()
    pos = m.positions()
    out["positions"] = pos
    out["kv"] = [[m.read_kv(l, b, int(pos[b])) for b in range(B)] for l in range(L)]
    return out


def _same(a, b, where="out"):
    """bit for bit, through the script's nested results"""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype, where
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
            (where, int(np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:1].sum()))
    else:
        assert a == b, (where, a, b)


def test_serving_paths_do_not_depend_on_where_pages_lie(hip):
    """prefill_ragged of 5, 70 and 130 tokens, score, a fork whose copied tail
    page (source and destination) holds a mark, three greedy verify rounds and
    a verify_tree round with accepted and rejected drafts, release and
    re-admission, six decode steps with log-probabilities: fp32, C = 768, graph
    on, on the default small pool and on the big one at the same B and max_ctx.
    Logits, ids, log-probabilities, accepted counts and read_kv rows are
    bit-identical.  (What the small-pool run computes is pinned against
    float64 by the dense-pass, speculation and decode modules.)"""
    C, NH, B, P, MAXC = INV["C"], INV["NH"], INV["B"], INV["P"], INV["MAX_CTX"]
    cfgd = dict(maxT=MAXC, V=INV["V"], L=ENGINE_L, NH=NH, C=C)
    params = synth.params(cfgd, seed=4242)
    tok = _inv_tokens()

    def small():
        m = hip.Model(cfgd, params=params)
        m.decode_init(B, P, MAXC)
        return m

    m = small()
    stream = _serve(hip, m, tok, greedy_steps=24)
    m.close()
    m = small()
    want = _serve(hip, m, tok, stream=stream)
    m.close()

    # the big pool: every page with a spare prompt, the zone pages freed stage by stage
    pb = pm.page_elems(NH, P) * 4
    N = pm.engine_pages(pb)
    need = B * -(-MAXC // P)
    keepers = -(-N // SPARE_PAGES)
    bm = hip.BlockManager(C, B + 3 + keepers, N, P, SPARE_PAGES)
    m = hip.Model(cfgd, params=params)
    m.set_manager(bm)
    _decode_init(hip, m, ENGINE_L * N * pb, B, P, MAXC)
    slots = m.page_slots(N).astype(np.int64)
    first = sum(-(-n // P) for n in INV["LENS"])  # 1 + 5 + 9 pages, handed out in this order
    stage1, dst, stage3, mk, (hold31, hold32) = plan_staged(slots, pb, need, first)
    owner = np.full(N, -1, np.int64)
    owner[stage1], owner[dst], owner[stage3] = B, B + 1, B + 2
    rest = np.flatnonzero(owner < 0)
    owner[rest] = B + 3 + np.arange(rest.size) // SPARE_PAGES
    L = hip.lib()
    for i, p in enumerate(owner.tolist()):
        blk = L.request_block(bm.h, p)
        assert blk and (i % 4096 or L.bm_block_index(bm.h, blk) == i), i
    assert bm.free_pages() == 0
    seen = {}

    def stage(name):
        if name == "fork":
            seen["before_fork"] = [slots[np.asarray(bm.pages(b), np.int64)].tolist() for b in range(B)]
            assert bm.free_pages() == 0  # the prefill and the score took exactly stage 1
        bm.free_prompt(B + ("prefill", "fork", "rest").index(name))

    got = _serve(hip, m, tok, stream=stream, stage=stage)
    pages = [slots[np.asarray(bm.pages(b), np.int64)].tolist() for b in range(B)]
    assert not m.evicted().any()
    m.close()
    bm.close()

    assert seen["before_fork"][2][-1] == hold32 and pages[3][8] == hold31, (seen["before_fork"][2], pages[3])
    assert pages[3][:8] == seen["before_fork"][2][:8]  # the full pages shared, the tail a copy
    allp = np.array(sorted({p for row in pages + seen["before_fork"] for p in row}), np.int64)
    for m_, (lo, hi) in pm.sides(allp, pb, mk).items():
        assert lo >= 1 and hi >= 1, m_
    accepted = [a for rnd in got["verify"] for a in rnd[0] if a is not None] + [a for a in got["tree"][0] if a is not None]
    assert max(accepted) >= 2 and min(accepted) <= 1, accepted  # accepted and rejected drafts both occurred
    print(f"POOLLARGE engine invariance layer={N * pb / pm.GiB:.3f}GiB x{ENGINE_L} pages={N}: fork tail copied from slot "
          f"{hold32} (holds 2^32 B) to slot {hold31} (holds 2^31 B); accepted per round "
          f"{[rnd[0] for rnd in got['verify']]} tree {got['tree'][0]} | {pm.describe(allp, pb, mk)}")
    _same(want, got)
