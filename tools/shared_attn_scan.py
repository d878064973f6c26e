#!/usr/bin/env python3
"""Shared-prefix decode attention at GPT-2 124M shapes (12 layers and heads,
page 16, context ~1000, fp32 pool) on forked engines: the feature on against
the feature off ON THE SAME FORKED ENGINE, which is what the caches already
give the plain kernel.  HIP events, warmed up, five samples per figure with on
and off alternating in one process: median (spread = max - min).

An engine is filled with `shared` random K/V tokens per slot
(gpt2_decode_fill_random), the non-leaders are released and forked from their
group's leader at `shared` tokens, and real decode steps grow every slot's own
suffix to the context.  Shapes: B = 64 as 1 x 64, 8 x 8, 32 x 2 forks and 64
unrelated sequences (empty plan), B = 8 as 1 x 8, all with 960 of ~1000 tokens
shared, and B = 64 as 1 x 64 with 256 shared.  Further shapes (--shapes) find
the thresholds: 512 and 768 shared tokens (1x64s512, 8x8s768, ...), B = 16 and
32 (1x16, 2x8, 1x32, 4x8), and 8 / 16 / 32 forks among 64 slots whose rest is
unrelated (1x8of64, 1x16of64, 1x32of64, 8x2of64).

1. us per attention launch (gpt2_decode_time_attention: 48 back-to-back
   launches walking over the 12 layers at the last step's positions), off
   against on with the plan forced (min_tiles 1, min_members 2, min_covered 2), at the picked
   prefix_splits and, with --splits, at forced ones.
2. the graph-replayed decode step, off against on, for 1 x 64 and 8 x 8.
usage: shared_attn_scan.py [--steps 200] [--splits 1,2,4,8] [--shapes 1x64,8x8,...] [--step-shapes 1x64,8x8]
HPA_LIB=<path> runs another build of the library (-DHPA_SHARED_NT=0: the
prefix tiles loaded with the default cache policy)."""
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
ap.add_argument("--splits", default="")
ap.add_argument("--shapes", default="1x64,8x8,32x2,64x1,1x8,1x64s256")
ap.add_argument("--step-shapes", default="1x64,8x8")
args = ap.parse_args()

P, MAXC, CTX, REPEATS, ITERS, WIN = 16, 1024, 1000, 5, 48, 20
# name: (B, forks per group, shared tokens, slots that take part in a group; the rest stay unrelated)
SHAPES = {"1x64": (64, 64, 960, 64), "8x8": (64, 8, 960, 64), "32x2": (64, 2, 960, 64), "64x1": (64, 1, 960, 64),
          "1x8": (8, 8, 960, 8), "1x64s256": (64, 64, 256, 64),
          # where the thresholds lie: shorter prefixes, smaller batches, a few forks among unrelated sequences
          "1x64s512": (64, 64, 512, 64), "1x64s768": (64, 64, 768, 64), "8x8s512": (64, 8, 512, 64),
          "8x8s768": (64, 8, 768, 64), "32x2s512": (64, 2, 512, 64), "32x2s768": (64, 2, 768, 64),
          "1x16": (16, 16, 960, 16), "1x32": (32, 32, 960, 32), "2x8": (16, 8, 960, 16), "4x8": (32, 8, 960, 32),
          "1x8of64": (64, 8, 960, 8), "1x16of64": (64, 16, 960, 16), "1x32of64": (64, 32, 960, 32),
          "8x2of64": (64, 2, 960, 16)}

pa.init(0)
print(f"# {pa.device_info()[0]}; library {os.path.relpath(pa.LIB_PATH, REPO)}")
print(f"# GPT-2 124M, page {P}, ctx {CTX}, fp32 pool; {REPEATS} samples, on and off alternating: "
      f"median (spread = max - min)")
t = pa.Timer()


def med(v):
    return statistics.median(v), max(v) - min(v)


def forked_engine(B, group, shared, forked):
    m = pa.Model(dict(pa.GPT2_124M), seed=1)
    m.decode_init(B, P, MAXC)
    m.fill_random(shared, seed=3)
    for b in range(B):
        if group > 1 and b % group and b < forked:
            m.release(b)
            m.fork(b - b % group, b, shared)
    m.set_graph(True)
    rng = np.random.default_rng(5)
    for _ in range(CTX - shared):  # every slot's own suffix, different tokens per slot
        m.step_async(rng.integers(0, 50257, B).astype(np.int32))
    m.status()
    return m


def attention_us(m, on, splits=0):
    m.set_shared_splits(splits)
    m.set_shared_attention(on, min_tiles=1, min_members=2, min_covered=2)
    m.shared_plan()
    m.time_attention(8)  # warm-up
    return m.time_attention(ITERS)[0] * 1e3


def step_ms(m, on, pos):
    m.set_shared_attention(on, min_tiles=1, min_members=2, min_covered=2)
    total, n = 0.0, -WIN
    while n < args.steps:
        m.set_positions(pos)
        m.shared_plan()  # the rewind's plan rebuild stays outside the window
        t.start()
        for _ in range(WIN):
            m.step_async()
        dt = t.stop()
        if n >= 0:  # the first window captures the graph
            total += dt
        n += WIN
    m.status()
    return total / n


for name in args.shapes.split(","):
    B, group, shared, forked = SHAPES[name]
    m = forked_engine(B, group, shared, forked)
    pos = m.positions().copy()
    m.set_shared_attention(True, min_tiles=1, min_members=2, min_covered=2)
    units, unit_of, tok = m.shared_plan()
    picked = m.shared_splits() if units else 0
    print(f"## {name}: B={B}, {forked} slots in groups of {group}, {shared} of {int(pos[0])} tokens shared; plan: {units} units, "
          f"{int((unit_of >= 0).sum())} members, {int(tok.max()) // 64} tiles, prefix_splits {picked} (picked); "
          f"off: splits {m.attn_splits()}, waves {m.attn_waves()}; layer form {m.layer_form()}")
    variants = [0] + ([int(x) for x in args.splits.split(",") if x] if units else [])
    res = {("off", 0): []}
    res.update({("on", s): [] for s in variants})
    for _ in range(REPEATS):
        for key, xs in res.items():
            xs.append(attention_us(m, key[0] == "on", key[1]))
    om, osp = med(res["off", 0])
    print(f"attention us/launch  off {om:7.2f} ({osp:5.2f})   repeats {' '.join(f'{x:.2f}' for x in res['off', 0])}")
    for s in variants:
        xm, xs = med(res["on", s])
        verdict = "wins" if om - xm > osp + xs else "loses" if xm - om > osp + xs else "inside the spreads"
        print(f"attention us/launch  on, prefix_splits {s or picked:2d}{' (picked)' if not s else '':9s} {xm:7.2f} "
              f"({xs:5.2f}) = {xm / om:5.3f} x off: {verdict}   repeats {' '.join(f'{x:.2f}' for x in res['on', s])}",
              flush=True)
    if name in args.step_shapes.split(","):
        m.set_shared_splits(0)
        off, on = [], []
        for _ in range(REPEATS):
            off.append(step_ms(m, False, pos))
            on.append(step_ms(m, True, pos))
        (fm, fs), (nm, ns) = med(off), med(on)
        verdict = "wins" if fm - nm > fs + ns else "loses" if nm - fm > fs + ns else "inside the spreads"
        print(f"decode step ms (graph)  off {fm:7.4f} ({fs:6.4f})   on {nm:7.4f} ({ns:6.4f}) = {nm / fm:5.3f} x off: "
              f"{verdict}")
        print(f"    repeats off {' '.join(f'{x:.4f}' for x in off)}")
        print(f"    repeats on  {' '.join(f'{x:.4f}' for x in on)}", flush=True)
    m.close()
