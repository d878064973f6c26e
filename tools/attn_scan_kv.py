#!/usr/bin/env python3
"""Decode attention and the whole decode step against the KV pool's storage
type: fp32, bf16 and fp8 (e4m3fn) pools of a synthetic GPT-2 124M, page 16,
context ~1020, B = 8 and 64.  Per pool and batch, repeated 5 times in this
process (median, and the spread max - min):
  * the attention launch alone (gpt2_decode_time_attention: back-to-back
    launches over the layers, HIP events), its algorithmic bytes and the
    fraction of 8 TB/s they make;
  * the graph-replayed step, ms per step over `steps` steps after a warm-up.
usage: attn_scan_kv.py [--steps N] [--sweep] [--batches 8,64] [--pools fp32,bf16,fp8]
--sweep adds, for the fp8 pool, the attention time at every waves x splits
(the engine's picks start from the bf16 rule; this is what they are set by).
HPA_LIB=<path> runs another build of the library (A/B builds)."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)  # <= 20: the warm-up is one window
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--batches", default="8,64")
ap.add_argument("--pools", default="fp32,bf16,fp8")
args = ap.parse_args()

CTX, P, REPEATS, HBM = 1024, 16, 5, 8e12
CHUNK = 20
FILL = CTX - 4 - CHUNK  # every timed window decodes positions 1000 .. 1019
POOLS = [(n, d) for n, d in (("fp32", pa.HPA_F32), ("bf16", pa.HPA_BF16), ("fp8", pa.HPA_FP8))
         if n in args.pools.split(",")]
BATCHES = [int(b) for b in args.batches.split(",")]

pa.init(0)
L = pa.lib()
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# GPT-2 124M synthetic, page {P}, fill {FILL}, {REPEATS} repeats: median (spread = max - min)")
m = pa.Model(dict(pa.GPT2_124M), seed=1)
t = pa.Timer()


def med(v):
    return statistics.median(v), max(v) - min(v)


def step_ms(B):
    """graph-replayed steps in windows of CHUNK steps from the filled state
    (positions FILL .. FILL + CHUNK - 1, rewound between windows, outside the
    timed span): ms per step over args.steps steps"""
    pos = np.full(B, FILL, np.int32)
    out = []
    for _ in range(REPEATS):
        m.set_positions(pos)
        for _ in range(args.warmup):
            m.step_async()
        total, n = 0.0, 0
        while n < args.steps:
            m.set_positions(pos)
            t.start()
            for _ in range(CHUNK):
                m.step_async()
            total += t.stop()
            n += CHUNK
        m.status()
        out.append(total / n)
    return out


rows = {}
for B in BATCHES:
    for name, dt in POOLS:
        m.decode_init(B, P, CTX, kv_dtype=dt)
        m.fill_random(FILL, seed=3)
        m.set_graph(True)
        m.step(np.zeros(B, np.int32))
        s_ms, s_sp = med(step_ms(B))  # leaves every sequence at position FILL + CHUNK = 1020
        att = [m.time_attention(48) for _ in range(REPEATS)]
        by = att[0][1]
        a_ms, a_sp = med([a[0] for a in att])
        rows[(B, name)] = (a_ms, a_sp)
        print(f"B={B:3d} {name:5s} form={m.layer_form()} splits={m.attn_splits():2d} waves={m.attn_waves()}  "
              f"attention {a_ms * 1e3:7.2f} us (spread {a_sp * 1e3:5.2f})  {by / 1e6:7.2f} MB  "
              f"{by / (a_ms * 1e-3) / HBM:5.3f} of 8 TB/s   step {s_ms:7.4f} ms (spread {s_sp:6.4f})", flush=True)
        if args.sweep and dt == pa.HPA_FP8:
            auto = m.attn_splits()
            for s in sorted({1, 2, 4, auto}):
                m.set_attn_splits(s)
                for w in (1, 2, 4, 8):
                    L.hpa_set_attention_waves(w)
                    v, sp = med([m.time_attention(48)[0] for _ in range(REPEATS)])
                    print(f"    fp8 sweep B={B:3d} splits={s:2d} waves={w}: {v * 1e3:7.2f} us (spread {sp * 1e3:5.2f})",
                          flush=True)
                L.hpa_set_attention_waves(0)
            m.set_attn_splits(0)
for B in BATCHES:
    if (B, "fp8") not in rows or (B, "bf16") not in rows:
        continue
    (f8, f8s), (bf, bfs) = rows[(B, "fp8")], rows[(B, "bf16")]
    print(f"B={B:3d}: fp8 attention {f8 * 1e3:.2f} us vs bf16 {bf * 1e3:.2f} us: {bf / f8:.2f}x, "
          f"difference {(bf - f8) * 1e3:.2f} us against spreads {f8s * 1e3:.2f} / {bfs * 1e3:.2f} us")
m.close()
