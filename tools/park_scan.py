"""Parking (profiles/r18/park.txt): GPT-2 124M, page 16, n = 1000 and n = 100
cached tokens, fp32 / bf16 / fp8 pools, B = 8.  Medians of 5 with max - min, the
variants alternating inside one process; wall clock (time.perf_counter) around
work that ends in hpa_synchronize, because the host link is what is measured.

(a) hpa_pool_gather_pages / hpa_pool_scatter_pages alone on a stand-alone pool
    (the sequence's pages scattered over 8 x 64 slots), three routes:
      direct      the kernel reads / writes pinned host memory itself, plain loads and stores
      direct_nt   the same with the pool side non-temporal (hpa_park_set_nontemporal; the default)
      staged      the kernel (default form) into / out of a device buffer + ONE hpa_memcpy_async
      staged+alloc  staged, with the device buffer's hpa_malloc and hpa_free inside the timing
                  (what an engine without a buffer cache would pay per call)
      copies      no kernel: one hpa_memcpy_async per (layer, page), the only
                  route before these kernels (issued from this script: the loop
                  carries one ctypes call per copy)
(b) gpt2_decode_park / gpt2_decode_unpark / gpt2_parked_free whole, and beside them
    hpa_host_alloc and hpa_host_free of the payload's size alone (the pinned
    allocation inside park, its release inside gpt2_parked_free)
(c) park + unpark against the route to the same state without them:
    gpt2_decode_release + gpt2_decode_prefill_ragged of the same n tokens

Usage: python tools/park_scan.py [out.txt]
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm.c-paged_amd"))
import numpy as np  # noqa: E402
import pagedattn as pa  # noqa: E402

pa.init(0)
L = pa.lib()
CFG = pa.GPT2_124M
LAYERS, NH, P, B, REPS = CFG["L"], CFG["NH"], 16, 8, 5
DTYPES = [("fp32", pa.HPA_F32), ("bf16", pa.HPA_BF16), ("fp8", pa.HPA_FP8)]
NS = (1000, 100)
DEFAULT_NT = L.hpa_park_nontemporal()
lines = [f"parking scan, {pa.device_info()[0]}",
         f"GPT-2 124M ({LAYERS} layers, {NH} heads), page {P}, B = {B}; median of {REPS} (max - min); wall clock to "
         f"hpa_synchronize", ""]


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def sync():
    pa.check(L.hpa_synchronize(), "synchronize")


def timed(fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e6


def stats(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[-1] - xs[0]


def alternate(variants, reps=REPS, warm=2):
    """variants: name -> callable; every repeat runs each variant once, in turn"""
    got = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            us = timed(fn)
            if r >= warm:
                got[k].append(us)
    return {k: stats(v) for k, v in got.items()}


# ------------------------------------------------------------------ (a) the kernels alone
say("(a) gather / scatter alone: us (spread) and GB/s of the payload, one direction")
for name, dt in DTYPES:
    pool = pa.Pool(LAYERS, NH, P, B * 64, dtype=dt)
    pb = pool.s.page_elems * pool.s.elem_bytes
    rng = np.random.default_rng(7)
    for n in NS:
        npg = -(-n // P)
        slots = np.ascontiguousarray(rng.permutation(B * 64)[:npg].astype(np.int32))
        nbytes = pool.park_bytes(npg)
        pin = pa.PinnedBuffer(nbytes)
        dev = pa.DeviceBuffer(nbytes)
        pin.array[:] = rng.integers(0, 256, nbytes, dtype=np.uint8)
        tiles = [[L.hpa_pool_tile(pool.ref, l, int(s), 0, 0) for s in slots] for l in range(LAYERS)]
        offs = [[pool.park_offset(npg, l, i) for i in range(npg)] for l in range(LAYERS)]

        def nt(mask, fn):
            def run():
                L.hpa_park_set_nontemporal(mask)
                fn()
                L.hpa_park_set_nontemporal(DEFAULT_NT)
            return run

        def with_alloc(gather):
            def run():
                d = L.hpa_malloc(nbytes)
                if gather:
                    pa.check(L.hpa_pool_gather_pages(pool.ref, slots.ctypes.data_as(pa._I), npg, d))
                    pa.check(L.hpa_memcpy_async(pin.ptr, d, nbytes))
                else:
                    pa.check(L.hpa_memcpy_async(d, pin.ptr, nbytes))
                    pa.check(L.hpa_pool_scatter_pages(pool.ref, slots.ctypes.data_as(pa._I), npg, d))
                sync()
                L.hpa_free(d)
            return run

        def g_staged():
            pool.gather_pages(slots, dev)
            pa.check(L.hpa_memcpy_async(pin.ptr, dev.ptr, nbytes))

        def s_staged():
            pa.check(L.hpa_memcpy_async(dev.ptr, pin.ptr, nbytes))
            pool.scatter_pages(slots, dev)

        def g_copies():
            for l in range(LAYERS):
                for i in range(npg):
                    L.hpa_memcpy_async(pin.ptr + offs[l][i], tiles[l][i], pb)

        def s_copies():
            for l in range(LAYERS):
                for i in range(npg):
                    L.hpa_memcpy_async(tiles[l][i], pin.ptr + offs[l][i], pb)

        res = alternate({"gather direct": nt(0, lambda: pool.gather_pages(slots, pin)),
                         "gather direct_nt": nt(1, lambda: pool.gather_pages(slots, pin)),
                         "gather staged": g_staged,
                         "gather staged+alloc": with_alloc(True),
                         "gather copies": g_copies,
                         "scatter direct": nt(0, lambda: pool.scatter_pages(slots, pin)),
                         "scatter direct_nt": nt(2, lambda: pool.scatter_pages(slots, pin)),
                         "scatter staged": s_staged,
                         "scatter staged+alloc": with_alloc(False),
                         "scatter copies": s_copies})
        say(f"  {name} n = {n}: {npg} pages x {LAYERS} layers x {pb} B = {nbytes / 1e6:.2f} MB")
        for k, (med, spread) in res.items():
            extra = f", {LAYERS * npg} copies" if k.endswith("copies") else ""
            say(f"    {k:20s} {med:9.1f} us ({spread:7.1f})  {nbytes / med / 1e3:7.2f} GB/s{extra}")
        pin.free()
        dev.free()
    pool.destroy()
say()

# ------------------------------------------------------------------ (b), (c) the engine calls
say("(b) gpt2_decode_park / gpt2_decode_unpark whole, sequence 0 of 8 live ones; pinned = hpa_host_alloc + hpa_host_free "
    "of the payload alone")
say("(c) park + unpark against gpt2_decode_release + gpt2_decode_prefill_ragged of the same n tokens (us; ratio = "
    "re-prefill / (park + unpark), > 1: parking wins)")
tok_rng = np.random.default_rng(11)
for name, dt in DTYPES:
    model = pa.Model(CFG, seed=1337)
    model.decode_init(B, P, CFG["maxT"], kv_dtype=dt)
    model.set_graph(True)
    for n in NS:
        model.reset()
        toks = [tok_rng.integers(0, CFG["V"], n).astype(np.int32) for _ in range(B)]
        for b in range(B):  # one sequence per pass: the workspace stays that of n rows
            model.prefill_ragged([toks[b] if i == b else [] for i in range(B)])
        model.step(None)  # a pending id of the engine's own, one more cached token
        state = {}

        def do_park():
            state["h"] = model.park(0)

        def do_unpark():
            model.unpark(state["h"], 0)

        def do_free():
            state["h"].free()

        def do_reprefill():
            model.release(0)
            model.prefill_ragged([np.concatenate([toks[0], toks[0][:1]])] + [[]] * (B - 1))

        probe = model.park(0, keep=True)
        nbytes, ntok = probe.bytes, probe.tokens
        probe.free()

        def do_pin_alloc():
            state["p"] = L.hpa_host_alloc(nbytes)

        def do_pin_free():
            L.hpa_host_free(state["p"])

        res = alternate({"park": do_park, "unpark": do_unpark, "free": do_free, "pin_alloc": do_pin_alloc,
                         "pin_free": do_pin_free, "release+prefill": do_reprefill})
        pk, un, fr, pa_, pf, rp = (res[k] for k in ("park", "unpark", "free", "pin_alloc", "pin_free", "release+prefill"))
        both, all3 = pk[0] + un[0], pk[0] + un[0] + fr[0]
        say(f"  {name} n = {ntok}: payload {nbytes / 1e6:.2f} MB")
        say(f"    park             {pk[0]:9.1f} us ({pk[1]:7.1f})   hpa_host_alloc of the payload alone "
            f"{pa_[0]:9.1f} us ({pa_[1]:7.1f}) = {pa_[0] / pk[0]:.2f} of park")
        say(f"    unpark           {un[0]:9.1f} us ({un[1]:7.1f})")
        say(f"    gpt2_parked_free {fr[0]:9.1f} us ({fr[1]:7.1f})   hpa_host_free of the payload alone  "
            f"{pf[0]:9.1f} us ({pf[1]:7.1f})")
        say(f"    release+prefill  {rp[0]:9.1f} us ({rp[1]:7.1f})")
        say(f"    park + unpark {both:9.1f} us: ratio {rp[0] / both:.2f};  with the handle's free {all3:9.1f} us: "
            f"ratio {rp[0] / all3:.2f};  without the pinned allocation and its release "
            f"{all3 - pa_[0] - pf[0]:9.1f} us: ratio {rp[0] / (all3 - pa_[0] - pf[0]):.2f}")
    model.close()

out = "\n".join(lines) + "\n"
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(out)
