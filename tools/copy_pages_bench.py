"""hpa_pool_copy_pages timing (profiles/r8/fork.txt): a GPT-2 124M fp32 page (P = 16, 12 layers), n = 1 and n = 64
pairs, HIP events around back-to-back launches.  Usage: python tools/copy_pages_bench.py [out.txt]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402

pa.init(0)
L = pa.lib()
LAYERS, NH, P, PAGES = 12, 12, 16, 1024
pool = pa.Pool(LAYERS, NH, P, PAGES)
page_bytes = pool.s.page_elems * pool.s.elem_bytes
pair_bytes = page_bytes * LAYERS
lines = [f"hpa_pool_copy_pages, {pa.device_info()[0]}",
         f"pool: fp32, {LAYERS} layers, {NH} heads, page {P}: {page_bytes} B per page per layer, "
         f"{pair_bytes} B per pair ({pair_bytes / 1e6:.3f} MB), {PAGES} pages ({pool.s.bytes / 1e9:.2f} GB)",
         "time: HIP events around ITERS back-to-back launches on one stream, after 10 warm-up launches;",
         "bytes = read + written = 2 * n * pair bytes; fraction of the 8 TB/s HBM peak",
         "rotate: each launch uses the next group of 2n pages of the pool (n = 64: 151 MB per launch, the",
         "        whole 1.2 GB pool before a page repeats: beyond the 256 MiB Infinity Cache); same: one",
         "        fixed set of pages every launch (cache-resident)", ""]
e0, e1 = L.hpa_event_create(), L.hpa_event_create()
ITERS = 64
for n in (1, 64):
    for mode in ("same", "rotate"):
        groups = PAGES // (2 * n) if mode == "rotate" else 1
        sets = []
        for g in range(groups):
            base = g * 2 * n
            s = np.arange(base, base + n, dtype=np.int32)
            d = np.arange(base + n, base + 2 * n, dtype=np.int32)
            sets.append((s, d, s.ctypes.data_as(pa._I), d.ctypes.data_as(pa._I)))
        for r in range(3):
            for k in range(10):
                s = sets[k % groups]
                pa.check(L.hpa_pool_copy_pages(pool.ref, s[2], s[3], n))
            pa.check(L.hpa_event_record(e0))
            for k in range(ITERS):
                s = sets[(10 + k) % groups]
                pa.check(L.hpa_pool_copy_pages(pool.ref, s[2], s[3], n))
            pa.check(L.hpa_event_record(e1))
            ms = L.hpa_event_elapsed_ms(e0, e1)
            us = ms * 1e3 / ITERS
            gbs = 2 * n * pair_bytes / (us * 1e-6) / 1e9
            lines.append(f"n = {n:2d} {mode:6s} run {r}: {us:8.2f} us per launch, {gbs:8.1f} GB/s, "
                         f"{gbs / 8000:.3f} of 8 TB/s")
out = "\n".join(lines) + "\n"
print(out)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(out)
pool.destroy()
