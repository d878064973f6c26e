"""The bf16 chain's host side, no GPU: the HpaChainB16Args struct mirror of
pagedattn against the header (sizeof and the offset of every member, from a
small C program built with the host compiler), the bound entry points, and the
numpy decoder of the bf16 fragment layout against the written formula.
"""
import ctypes
import os
import re
import subprocess

import numpy as np

import pagedattn as pa

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_args_mirror_matches_the_header(tmp_path):
    names = [n for n, _ in pa.HpaChainB16Args._fields_]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hip_paged_attn.h"\n'
                   'int main(void) {\n    printf("%zu\\n", sizeof(HpaChainB16Args));\n'
                   + "".join(f'    printf("{n} %zu %zu\\n", offsetof(HpaChainB16Args, {n}), '
                             f'sizeof(((HpaChainB16Args*)0)->{n}));\n' for n in names)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "off")
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe],
                   check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert ctypes.sizeof(pa.HpaChainB16Args) == int(lines[0])
    end = 0
    for n, line in zip(names, lines[1:]):
        name, off, size = line.split()
        f = getattr(pa.HpaChainB16Args, n)
        assert (name, int(off), int(size)) == (n, f.offset, f.size), line
        assert int(off) >= end  # the header's member order
        end = int(off) + int(size)
    # every member of the header's struct is mirrored: nothing but padding is left over
    hdr = open(os.path.join(REPO, "include", "hip_paged_attn.h")).read()
    body = hdr[:hdr.index("} HpaChainB16Args;")]
    body = body[body.rindex("typedef struct {") + len("typedef struct {"):]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split(";"):
        for piece in stmt.split(","):
            m = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", piece.strip())
            if m:
                declared.append(m.group(1))
    assert declared == names


def test_chain_entry_points_are_bound():
    L = pa.lib()
    for name in ("hpa_decode_chain_b16", "hpa_decode_chain_b16_first", "hpa_decode_chain_b16_sizes",
                 "hpa_decode_chain_b16_eligible"):
        assert getattr(L, name).argtypes is not None
    # pure host arithmetic: a unit per workgroup on 256 CUs up to 256 rows, not on 128
    assert L.hpa_decode_chain_b16_eligible_cus(256, 768, 12, 256) == 1
    assert L.hpa_decode_chain_b16_eligible_cus(256, 768, 12, 128) == 0
    assert L.hpa_decode_chain_b16_eligible_cus(257, 768, 12, 256) == 0
    out = (ctypes.c_size_t * 2)()
    assert L.hpa_decode_chain_b16_sizes(72, out) == 0
    assert list(out) == [4 * 2 * 16 * 4 * 3 * 256, 160 * 32]


def test_from_frag_bf16_follows_the_written_formula():
    """element (m, k) at ((m/16 * K/32 + k/32) * 64 + m%16 + 16*((k%16)/4)) * 8 + k%4
    + 4*((k%32)/16) (include/hip_paged_attn.h), on an index pattern: plain loops"""
    rows, K = 48, 96
    buf = np.arange(rows * K, dtype=np.uint16) * 3 + 1
    got = pa.from_frag_bf16(buf, rows, K)
    assert got.shape == (rows, K) and got.dtype == np.uint16
    seen = set()
    for m in range(rows):
        for k in range(K):
            i = ((m // 16 * (K // 32) + k // 32) * 64 + m % 16 + 16 * ((k % 16) // 4)) * 8 + k % 4 + 4 * ((k % 32) // 16)
            assert got[m, k] == buf[i], (m, k)
            seen.add(i)
    assert seen == set(range(rows * K))  # a permutation of the buffer
    # the fc epilogue's form of the same address (hpa_chain_b16.hip): bytes
    for m, k in ((0, 0), (17, 36), (47, 95), (33, 52)):
        lt = (m & 15) + 16 * ((k & 15) >> 2)
        off = (((m >> 4) * (K // 32) + (k >> 5)) * 64 + lt) * 16 + ((k >> 4) & 1) * 8
        assert off // 2 + (k & 3) == pa.frag_bf16_index(m, k, K)
    # fewer rows than the buffer holds: the padded rows are left out
    assert np.array_equal(pa.from_frag_bf16(buf, 40, K), got[:40])
