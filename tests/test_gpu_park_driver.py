"""examples/decode_main.c --park-at N: every sequence is parked after N generated
tokens, the pool is shown empty, every sequence is unparked one slot on -- and
the driver prints the text and writes the ids of the run without the flag
(greedy, and sampled: the sampler state travels with the sequence)."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_integration as tgi

pytestmark = pytest.mark.gpu
GOLD = tgi.GOLD


def _generated_text(stdout):
    body = stdout.split(b"generating:\n---\n", 1)[1]
    return body.split(b"\n---\nFinished!", 1)[0]


@pytest.mark.parametrize("mode", ["greedy", "sampled", "filtered"])
def test_park_at_prints_the_same_text(hip, tmp_path, mode):
    exe = tgi._build_driver(tmp_path)
    exp = np.load(os.path.join(GOLD, "ckpt_expected.npz"))
    B, P, N = 3, 8, 16
    prompts = exp["tokens"][:B * P].astype(np.int32).reshape(B, P)
    tok_file = tmp_path / "tokens.bin"
    prompts.tofile(tok_file)
    flags = {"greedy": ["-g"], "sampled": [], "filtered": ["--temperature", "0.9", "--top-k", "50"]}[mode]
    runs = []
    for park in ([], ["--park-at", "9"]):  # 17 cached tokens: two pages of 16, the second partly filled
        ids_file = tmp_path / f"ids{len(park)}.bin"
        args = [exe, "-c", os.path.join(GOLD, "ckpt_v1.bin"), "-k", os.path.join(GOLD, "tokenizer.bin"), "-t",
                str(tok_file), "-b", str(B), "-p", str(P), "-n", str(N), "-o", str(ids_file)] + flags + park
        r = subprocess.run(args, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        runs.append((np.fromfile(ids_file, np.int32).reshape(B, P + N), _generated_text(r.stdout), r.stderr))
    (ids0, text0, err0), (ids1, text1, err1) = runs
    assert np.array_equal(ids0, ids1), (ids0, ids1)
    assert text0 == text1 and len(text0) > 0
    pages = B * -(-(P + N) // 16)
    assert f"{pages} of {pages} pages free".encode() in err1 and b"parked" not in err0
    # a slot mix-up would show wherever the sequences differ: each draws from its own stream when sampling
    # (greedy, this small checkpoint continues all three prompts alike, so only the rows' prompts differ there)
    assert len({ids0[b].tobytes() for b in range(B)}) == B
    if mode != "greedy":
        assert len({ids0[b, P:].tobytes() for b in range(B)}) == B


def test_park_at_is_checked(tmp_path):
    """refused before anything is built: N outside 1..new_tokens - 1, or a --speculate flag"""
    exe = tgi._build_driver(tmp_path)
    for extra in (["--park-at", "0"], ["--park-at", "4"], ["--park-at", "2", "-g", "--speculate", "2"]):
        r = subprocess.run([exe, "-b", "2", "-p", "4", "-n", "4"] + extra, capture_output=True, timeout=60)
        assert r.returncode == 2 and b"--park-at" in r.stderr, (extra, r.stderr)
