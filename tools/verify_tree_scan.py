#!/usr/bin/env python3
"""Tree speculation at GPT-2 124M shapes (12 heads, page 16, context ~1000,
fp32 pool).  HIP events, warmed up, five samples per figure with the versions
alternating in one process: median (spread = max - min).

1. The tree attention against the chain attention: us per launch of
   hpa_paged_attention_verify (the chain kernel) and of
   hpa_paged_attention_verify_tree with chain masks and with star masks, on the
   same inputs, B = 8 and 64, 4 and 8 rows per sequence.  20 back-to-back
   launches per sample, walking over 64 / B copies of the batch in different
   pages so that every launch streams from HBM (tools/verify_scan.py).
2. hpa_pool_compact_path alone, 12 layers, B = 64: the path (3, 5, 7) -- three
   moved rows per sequence, sources in the next page -- and (2, 3, 4, 5, 6, 7)
   -- six, the most a pass of 8 nodes can move: a path of 7 is the chain and
   moves nothing -- and a = 0 (the launch alone).
3. A whole gpt2_decode_verify_tree pass of 8 nodes (a star of 7 drafts) against
   gpt2_decode_verify of 8 rows on the same engine, host-synchronous wall
   clock, and the graph-replayed decode step; the break-even accepted depth of
   a tree pass from the two.  The drafts are arbitrary ids, so both passes
   accept nothing and the compaction launch moves nothing: the difference is
   the row-table kernel, the targets' fill, the accept walk, the compaction
   launch and the larger tables; what moving rows adds is part 2.
usage: verify_tree_scan.py [--steps 200]
HPA_LIB=<path> runs another build of the library."""
import argparse
import ctypes
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
args = ap.parse_args()

NH, HS, P, CTX, REPEATS, LAUNCHES, NL = 12, 64, 16, 1000, 5, 20, 12
C = NH * HS
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_U8 = ctypes.POINTER(ctypes.c_ubyte)

pa.init(0)
L = pa.lib()
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# GPT-2 124M heads, page {P}, ctx {CTX}, fp32 pool; {REPEATS} samples: median (spread = max - min)")
t = pa.Timer()
rng = np.random.default_rng(0)


def med(v):
    return statistics.median(v), max(v) - min(v)


def fi(buf):
    return ctypes.cast(buf.ptr, _I)


def ff(buf):
    return ctypes.cast(buf.ptr, _F)


def sample(fn, n=LAUNCHES):
    t.start()
    for i in range(n):
        fn(i)
    return t.stop() * 1e3 / n


# ---- 1. the attention kernels
print(f"# 1. attention, us per launch, {LAUNCHES} launches per sample")
for B in (64, 8):
    nsets = max(1, 64 // B)
    npg = (CTX + P - 1) // P
    pool = pa.Pool(1, NH, P, nsets * B * npg)
    tables = rng.permutation(nsets * B * npg).astype(np.int32).reshape(nsets, B, npg)
    d_bt = [pa.DeviceBuffer.from_array(np.ascontiguousarray(tables[s])) for s in range(nsets)]
    for s in range(nsets):
        pa.check(L.hpa_pool_fill_random(pool.ref, d_bt[s].ptr, npg, B, CTX, 7 + s), "fill")
    for rows in (4, 8):
        R = B * rows
        d_q = pa.DeviceBuffer.from_array(rng.uniform(-1, 1, (R, C)).astype(np.float32))
        d_out = pa.DeviceBuffer((R + 15) // 16 * 16 * C * 4)
        d_start = pa.DeviceBuffer.from_array(np.full(B, CTX - rows, np.int32))
        d_row0 = pa.DeviceBuffer.from_array((np.arange(B) * rows).astype(np.int32))
        d_len = pa.DeviceBuffer.from_array(np.full(B, rows, np.int32))
        chain_m = np.tile(np.array([(2 << r) - 1 for r in range(rows)], np.uint8), B)
        star_m = np.tile(np.array([1 | (1 << r) for r in range(rows)], np.uint8), B)
        d_chain, d_star = pa.DeviceBuffer.from_array(chain_m), pa.DeviceBuffer.from_array(star_m)

        def chain(i):
            pa.check(L.hpa_paged_attention_verify(ff(d_q), pool.ref, 0, fi(d_bt[i % nsets]), npg, fi(d_start),
                                                  fi(d_row0), fi(d_len), B, rows, ff(d_out)), "verify")

        def tree(masks):
            def fn(i):
                pa.check(L.hpa_paged_attention_verify_tree(ff(d_q), pool.ref, 0, fi(d_bt[i % nsets]), npg, fi(d_start),
                                                           fi(d_row0), fi(d_len), ctypes.cast(masks.ptr, _U8), B, rows,
                                                           ff(d_out)), "verify_tree")
            return fn

        fns = (chain, tree(d_chain), tree(d_star))
        for fn in fns:  # warm-up: code objects, clocks
            for i in range(4):
                fn(i)
        pa.check(L.hpa_synchronize())
        v = [[], [], []]
        for _ in range(REPEATS):
            for k, fn in enumerate(fns):
                v[k].append(sample(fn))
        (cm, cs), (tm, ts), (sm, ss) = med(v[0]), med(v[1]), med(v[2])
        print(f"B={B:3d} rows={rows}: chain kernel {cm:7.2f} us ({cs:5.2f})   tree kernel, chain masks {tm:7.2f} us "
              f"({ts:5.2f}) = {tm / cm:5.3f} x   tree kernel, star masks {sm:7.2f} us ({ss:5.2f}) = {sm / cm:5.3f} x   "
              f"chain-mask difference {tm - cm:+.2f} us is {'inside' if abs(tm - cm) <= max(cs, ts) else 'outside'} "
              f"the spread", flush=True)
        for name, xs in zip(("chain kernel", "tree, chain", "tree, star "), v):
            print(f"    repeats {name} {' '.join(f'{x:.2f}' for x in xs)}")
        for b in (d_q, d_out, d_start, d_row0, d_len, d_chain, d_star):
            b.free()
    for b in d_bt:
        b.free()
    del pool

# ---- 2. the compaction launch alone
print(f"# 2. hpa_pool_compact_path, {NL} layers, B = 64, us per launch, {LAUNCHES} launches per sample "
      f"(hpa_pool_copy_pages, 64 pages of the same pool shape: 38-44 us, profiles/r8/fork.txt)")
B, npg, nsets = 64, 4, 4
pool = pa.Pool(NL, NH, P, nsets * B * npg)
tables = rng.permutation(nsets * B * npg).astype(np.int32).reshape(nsets, B, npg)
d_bt = [pa.DeviceBuffer.from_array(np.ascontiguousarray(tables[s])) for s in range(nsets)]
d_start = pa.DeviceBuffer.from_array(np.full(B, 13, np.int32))  # slots 13 .. 20: the page edge at 16
res = []
for name, path in (("a = 0", []), ("3 rows (3, 5, 7)", [3, 5, 7]), ("6 rows (2 .. 7)", [2, 3, 4, 5, 6, 7])):
    hp = np.zeros((B, pa.VERIFY_MAX_ROWS), np.int32)
    hp[:, :len(path)] = path
    d_path = pa.DeviceBuffer.from_array(hp)
    d_acc = pa.DeviceBuffer.from_array(np.full(B, len(path), np.int32))

    def compact(i, d_path=d_path, d_acc=d_acc):
        pa.check(L.hpa_pool_compact_path(pool.ref, fi(d_bt[i % nsets]), npg, fi(d_start), fi(d_path), fi(d_acc), B),
                 "compact_path")
    res.append((name, compact, []))
for _, fn, _ in res:
    for i in range(4):
        fn(i)
pa.check(L.hpa_synchronize())
for _ in range(REPEATS):
    for _, fn, xs in res:
        xs.append(sample(fn))
for name, _, xs in res:
    m_, s_ = med(xs)
    moved = 0 if name.startswith("a") else int(name.split()[0]) * B * NL * 2 * C * 4
    print(f"compact_path {name:18s}: {m_:7.2f} us ({s_:5.2f})   {moved / 1e6:6.2f} MB moved   "
          f"repeats {' '.join(f'{x:.2f}' for x in xs)}", flush=True)
del pool

# ---- 3. a whole tree pass of 8 nodes against a chain pass of 8 rows and the decode step
print("# 3. whole passes, ms (host-synchronous wall clock), and the graph-replayed decode step")
MAXC, WIN = 1024, 20
FILL = MAXC - 8 - WIN
for B in (64, 8):
    m = pa.Model(dict(pa.GPT2_124M), seed=1)
    m.decode_init(B, P, MAXC)
    m.fill_random(FILL, seed=3)
    m.set_graph(True)
    m.step(np.zeros(B, np.int32))  # a valid pending id per sequence
    pos = np.full(B, FILL, np.int32)
    ids = [11, 12, 13, 14, 15, 16, 17]
    drafts = [ids] * B
    trees = [(ids, [0] * 7)] * B

    def step_ms():
        m.set_positions(pos)
        for _ in range(WIN):
            m.step_async()
        total, n = 0.0, 0
        while n < args.steps:
            m.set_positions(pos)
            t.start()
            for _ in range(WIN):
                m.step_async()
            total += t.stop()
            n += WIN
        m.status()
        return total / n

    def pass_ms(fn, arg):
        for _ in range(3):
            m.set_positions(pos)
            fn(arg)
        total, n, acc = 0.0, 0, 0
        while n < max(20, args.steps // 10):
            m.set_positions(pos)
            t0 = time.perf_counter()
            a = fn(arg)[0]
            total += (time.perf_counter() - t0) * 1e3
            acc += sum(a)
            n += 1
        return total / n, acc / (n * B)

    st, pc, pt, ac, at = [], [], [], [], []
    for _ in range(REPEATS):
        st.append(step_ms())
        x, a = pass_ms(m.verify, drafts)
        pc.append(x)
        ac.append(a)
        x, a = pass_ms(m.verify_tree, trees)
        pt.append(x)
        at.append(a)
    (sm, ss), (cm, cs), (tm, ts) = med(st), med(pc), med(pt)
    print(f"B={B:3d} ctx~{FILL}: decode step (graph, form {m.layer_form()}) {sm:7.4f} ms ({ss:6.4f})   "
          f"chain pass, 8 rows {cm:7.4f} ms ({cs:6.4f})   tree pass, 8 nodes {tm:7.4f} ms ({ts:6.4f})   "
          f"tree - chain {tm - cm:+.4f} ms, tree / chain {tm / cm:5.3f}   "
          f"tree pass / step {tm / sm:4.2f}: break-even at {tm / sm - 1:4.2f} accepted drafts per pass "
          f"(chain pass: {cm / sm - 1:4.2f})   mean accepted: chain {statistics.mean(ac):.2f}, tree "
          f"{statistics.mean(at):.2f}", flush=True)
    print(f"    repeats step  {' '.join(f'{x:.4f}' for x in st)}")
    print(f"    repeats chain {' '.join(f'{x:.4f}' for x in pc)}")
    print(f"    repeats tree  {' '.join(f'{x:.4f}' for x in pt)}", flush=True)
    m.close()
