"""Refcounted pages of the block manager (bm_fork_prompt and friends), host
logic only (pages from host malloc, no GPU): a prompt forks another's prefix,
eviction skips shared pages and hands them to the remaining holder, release
order does not matter, bad arguments change nothing.  The same scenarios run
once more as a stand-alone C program that #includes block_manager.c and is
compiled with -fsanitize=address,undefined.

tests/test_block_manager.py (golden trace, the reference's own test) stays the
evidence that a manager that never forks behaves as before.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 4  # channels: page payloads are 16 * 4 floats


@pytest.fixture(scope="module")
def pa():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "llm.c-paged_amd"), "-j8"], check=True)
    import pagedattn
    pagedattn.lib()
    return pagedattn


def manager(pa, prompts, pages, per_prompt=None):
    return pa.BlockManager(C, max_prompts=prompts, max_blocks=pages, block_size=16,
                           max_blocks_per_prompt=per_prompt or pages, host_pages=True)


def snapshot(bm):
    s = bm.struct()
    return dict(lists=[bm.pages(p) for p in range(s.max_prompts)],
                refs=[bm.refs(i) for i in range(s.max_blocks)],
                owner=[bm.block(i).prompt_id for i in range(s.max_blocks)],
                lru=[bm.block(i).lru_counter for i in range(s.max_blocks)],
                free=bm.free_pages(), shared=bm.shared_pages(), epoch=s.lru_epoch)


def forked_3x6(pa):
    """case 1: prompt 0 holds pages 0, 1, 2; prompt 1 shares 0, 1 and owns 3;
    prompt 2 owns 4, 5; the pool is full"""
    bm = manager(pa, 3, 6)
    assert [bm.request_block(0) for _ in range(3)] == [0, 1, 2]
    bm.fork(0, 1, 2)
    assert bm.pages(1) == [0, 1]
    assert [bm.refs(i) for i in range(6)] == [2, 2, 1, 0, 0, 0]
    assert bm.shared_pages() == 2 and bm.free_pages() == 3
    assert bm.struct().dirty_lo <= 1 <= bm.struct().dirty_hi
    # the pages themselves are untouched by a fork
    assert [bm.block(i).prompt_id for i in range(3)] == [0, 0, 0]
    assert [bm.block(i).lru_counter for i in range(3)] == [1, 2, 3]
    assert bm.request_block(1) == 3
    assert [bm.request_block(2) for _ in range(2)] == [4, 5]
    assert bm.free_pages() == 0
    return bm


def test_fork_bookkeeping(pa):
    bm = forked_3x6(pa)
    assert bm.pages(0) == [0, 1, 2] and bm.pages(1) == [0, 1, 3] and bm.pages(2) == [4, 5]
    assert [bm.refs(i) for i in range(6)] == [2, 2, 1, 1, 1, 1]
    assert bm.refs(-1) == 0 and bm.refs(6) == 0
    bm.close()


def test_eviction_skips_shared_pages_and_hands_them_over(pa):
    bm = forked_3x6(pa)
    # pool full: the LRU page with ONE holder is prompt 0's page 2 (pages 0 and 1 are older but shared)
    assert bm.request_block(2) == 2
    assert bm.last_evicted() == 0
    assert bm.pages(0) == []
    assert [bm.refs(i) for i in range(6)] == [1, 1, 1, 1, 1, 1]
    assert bm.block(0).prompt_id == 1 and bm.block(1).prompt_id == 1 and bm.block(2).prompt_id == 2
    assert bm.shared_pages() == 0 and bm.free_pages() == 0
    assert bm.pages(1) == [0, 1, 3] and bm.pages(2) == [4, 5, 2]
    # now page 0 is private and the oldest: prompt 1 goes, whole (3 pages freed, 1 taken)
    assert bm.request_block(2) == 0
    assert bm.last_evicted() == 1
    assert bm.pages(1) == [] and bm.pages(2) == [4, 5, 2, 0]
    assert bm.free_pages() == 2
    assert [bm.refs(i) for i in range(6)] == [1, 0, 1, 0, 1, 1]
    bm.close()


def test_all_pages_shared_evicts_nobody(pa):
    bm = manager(pa, 2, 2, per_prompt=4)
    assert [bm.request_block(0) for _ in range(2)] == [0, 1]
    bm.fork(0, 1, 2)
    before = snapshot(bm)
    assert bm.request_block(0) == -1  # "No blocks available."
    assert bm.last_evicted() == -1
    assert snapshot(bm) == before
    assert bm.request_block(1) == -1
    assert snapshot(bm) == before
    bm.close()


@pytest.mark.parametrize("first", [0, 1])
def test_release_order(pa, first):
    bm = manager(pa, 3, 6)
    for _ in range(3):
        bm.request_block(0)
    bm.fork(0, 1, 2)
    bm.request_block(1)
    second = 1 - first
    bm.free_prompt(first)
    # the shared pages stay allocated, named after the holder that is left
    assert bm.pages(second)[:2] == [0, 1]
    assert [bm.refs(0), bm.refs(1)] == [1, 1] and bm.shared_pages() == 0
    assert bm.block(0).prompt_id == second and bm.block(1).prompt_id == second
    assert bm.block(0).keys and bm.block(1).values
    assert bm.free_pages() == 6 - 3
    bm.free_prompt(second)
    assert bm.free_pages() == 6
    assert [bm.refs(i) for i in range(6)] == [0] * 6
    assert [bm.block(i).prompt_id for i in range(6)] == [-1] * 6
    # a freed shared page is handed out again like any other
    assert bm.request_block(2) == 0
    bm.close()


def test_destroy_with_live_shared_pages(pa):
    bm = manager(pa, 3, 6)
    for _ in range(3):
        bm.request_block(0)
    bm.fork(0, 1, 3)
    bm.fork(0, 2, 1)
    assert [bm.refs(i) for i in range(3)] == [3, 2, 2] and bm.shared_pages() == 3
    bm.close()  # every payload released once (the sanitizer program checks the same under ASan)


def test_three_holders_hand_over_to_the_lowest(pa):
    bm = manager(pa, 4, 6)
    bm.request_block(1)
    bm.fork(1, 3, 1)
    bm.fork(1, 2, 1)
    assert bm.refs(0) == 3 and bm.block(0).prompt_id == 1
    bm.free_prompt(1)
    assert bm.refs(0) == 2 and bm.block(0).prompt_id == 2 and bm.shared_pages() == 1
    bm.free_prompt(3)  # not the named holder: the name stays
    assert bm.refs(0) == 1 and bm.block(0).prompt_id == 2 and bm.shared_pages() == 0
    bm.close()


def test_bad_arguments_change_nothing(pa):
    bm = manager(pa, 3, 6, per_prompt=2)
    bm.request_block(0)
    bm.request_block(0)
    bm.request_block(1)
    before = snapshot(bm)
    for src, dst, n in [(0, 1, 1),    # dst owns a page
                        (0, 2, 3),    # more pages than src has
                        (0, 2, -1),
                        (-1, 2, 0), (3, 2, 0), (0, -1, 1), (0, 3, 1),  # ids out of range
                        (0, 0, 1), (2, 2, 0)]:  # src == dst
        with pytest.raises(ValueError):
            bm.fork(src, dst, n)
        assert snapshot(bm) == before, (src, dst, n)
    bm.fork(0, 2, 0)  # an empty prefix is legal and shares nothing
    assert bm.pages(2) == [] and bm.shared_pages() == 0
    bm.close()


def test_make_private_swaps_in_a_fresh_page(pa):
    """bm_make_private (the engine's rewind guard): the shared page at one index
    of one holder's list is replaced by a fresh page; the others keep it"""
    import ctypes
    L = pa.lib()
    bm = manager(pa, 3, 6)
    for _ in range(3):
        bm.request_block(0)
    bm.fork(0, 1, 2)
    old = ctypes.c_int(-7)
    assert L.bm_make_private(bm.h, 1, 0, ctypes.byref(old)) == 3 and old.value == 0
    assert bm.pages(1) == [3, 1] and bm.pages(0) == [0, 1, 2]
    assert [bm.refs(i) for i in range(4)] == [1, 2, 1, 1] and bm.shared_pages() == 1
    assert bm.block(3).prompt_id == 1 and bm.block(0).prompt_id == 0
    # a private page is left where it is
    assert L.bm_make_private(bm.h, 1, 0, ctypes.byref(old)) == 3 and old.value == 3
    assert L.bm_make_private(bm.h, 0, 2, None) == 2
    # the named holder makes its copy: the name moves to the other holder
    assert L.bm_make_private(bm.h, 0, 1, None) == 4
    assert bm.block(1).prompt_id == 1 and bm.refs(1) == 1 and bm.shared_pages() == 0
    assert L.bm_make_private(bm.h, 0, 3, None) == -1 and L.bm_make_private(bm.h, 5, 0, None) == -1
    bm.close()
    # pool full and every other page shared: no page to copy into, nothing changes
    bm = manager(pa, 2, 2, per_prompt=4)
    bm.request_block(0)
    bm.request_block(0)
    bm.fork(0, 1, 2)
    before = snapshot(bm)
    assert L.bm_make_private(bm.h, 1, 0, None) == -1
    assert snapshot(bm) == before
    bm.close()


SANITIZER_PROGRAM = r"""
#include <assert.h>
#include "block_manager.c"

static int idx(BlockManager* m, KVBlock* b) { return b ? bm_block_index(m, b) : -1; }
static int req(BlockManager* m, int p) { return idx(m, request_block(m, p)); }

static BlockManager* forked_3x6(void) { /* case 1 */
    BlockManager* m = create_block_manager_ex(4, 3, 6, 16, 6);
    assert(m);
    assert(req(m, 0) == 0 && req(m, 0) == 1 && req(m, 0) == 2);
    assert(bm_fork_prompt(m, 0, 1, 2) == 0);
    assert(m->prompt_block_count[1] == 2 && m->prompt_block_list[1][0] == 0 && m->prompt_block_list[1][1] == 1);
    assert(bm_page_refs(m, 0) == 2 && bm_page_refs(m, 1) == 2 && bm_page_refs(m, 2) == 1);
    assert(bm_shared_pages(m) == 2 && bm_free_pages(m) == 3);
    assert(req(m, 1) == 3 && req(m, 2) == 4 && req(m, 2) == 5);
    assert(bm_free_pages(m) == 0);
    return m;
}

int main(void) {
    BlockManager* m = forked_3x6();
    /* case 2: eviction skips the shared pages and hands them over */
    m->blocks[0].keys[0] = 1.5f; /* the payload stays alive through the hand-over */
    assert(req(m, 2) == 2 && m->last_evicted_prompt == 0);
    assert(m->prompt_block_count[0] == 0);
    assert(bm_page_refs(m, 0) == 1 && bm_page_refs(m, 1) == 1 && bm_shared_pages(m) == 0);
    assert(m->blocks[0].prompt_id == 1 && m->blocks[1].prompt_id == 1);
    assert(m->blocks[0].keys[0] == 1.5f);
    assert(m->prompt_block_count[1] == 3 && m->prompt_block_list[1][0] == 0 && m->prompt_block_list[1][1] == 1 &&
           m->prompt_block_list[1][2] == 3);
    assert(req(m, 2) == 0 && m->last_evicted_prompt == 1);
    assert(bm_free_pages(m) == 2 && m->prompt_block_count[1] == 0);
    destroy_block_manager(m);

    /* case 3: all pages shared */
    m = create_block_manager_ex(4, 2, 2, 16, 4);
    assert(req(m, 0) == 0 && req(m, 0) == 1);
    assert(bm_fork_prompt(m, 0, 1, 2) == 0);
    assert(request_block(m, 0) == NULL && m->last_evicted_prompt == -1);
    assert(bm_page_refs(m, 0) == 2 && bm_page_refs(m, 1) == 2 && bm_free_pages(m) == 0);
    assert(m->prompt_block_count[0] == 2 && m->prompt_block_count[1] == 2);
    assert(bm_make_private(m, 1, 0, NULL) == -1 && bm_page_refs(m, 0) == 2);
    destroy_block_manager(m); /* live shared pages: every payload released once */

    /* case 4: release order, both ways */
    for (int first = 0; first < 2; first++) {
        const int second = 1 - first;
        m = create_block_manager_ex(4, 3, 6, 16, 6);
        req(m, 0); req(m, 0); req(m, 0);
        assert(bm_fork_prompt(m, 0, 1, 2) == 0);
        req(m, 1);
        m->blocks[1].values[63] = 2.5f;
        free_blocks_for_prompt(m, first);
        assert(bm_page_refs(m, 0) == 1 && bm_page_refs(m, 1) == 1 && bm_shared_pages(m) == 0);
        assert(m->blocks[0].prompt_id == second && m->blocks[1].prompt_id == second);
        assert(m->blocks[1].values[63] == 2.5f);
        assert(bm_free_pages(m) == 3);
        free_blocks_for_prompt(m, second);
        assert(bm_free_pages(m) == 6 && bm_page_refs(m, 0) == 0);
        destroy_block_manager(m);
    }

    /* the rewind guard's swap: the old page keeps its payload for the other holder */
    m = create_block_manager_ex(4, 3, 6, 16, 6);
    req(m, 0); req(m, 0); req(m, 0);
    assert(bm_fork_prompt(m, 0, 1, 2) == 0 && bm_fork_prompt(m, 0, 2, 1) == 0);
    int old = -1;
    assert(bm_make_private(m, 0, 0, &old) == 3 && old == 0);
    m->blocks[3].keys[0] = m->blocks[0].keys[0] = 3.0f;
    assert(bm_page_refs(m, 0) == 2 && m->blocks[0].prompt_id == 1 && m->blocks[3].prompt_id == 0);
    destroy_block_manager(m);

    /* bad arguments */
    m = create_block_manager_ex(4, 3, 6, 16, 2);
    req(m, 0); req(m, 1);
    assert(bm_fork_prompt(m, 0, 1, 1) && bm_fork_prompt(m, 0, 2, 2) && bm_fork_prompt(m, 0, 0, 1) &&
           bm_fork_prompt(m, 3, 2, 0) && bm_fork_prompt(m, 0, -1, 0) && bm_fork_prompt(m, 0, 2, -1));
    assert(bm_shared_pages(m) == 0 && bm_free_pages(m) == 4 && m->prompt_block_count[2] == 0);
    free(m->blocks[0].keys); free(m->blocks[0].values); free(m->blocks[1].keys); free(m->blocks[1].values);
    free(m); /* the reference idiom: one block holds the manager, page_refs included */
    return 0;
}
"""


def test_standalone_sanitizer_program(tmp_path):
    """cases 1 to 4 replayed by a C program of its own (own main, block_manager.c
    #included textually as the reference's callers do) under ASan + UBSan"""
    src = tmp_path / "bm_share.c"
    src.write_text(SANITIZER_PROGRAM)
    exe = tmp_path / "bm_share"
    r = subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "include"),
                        "-iquote", os.path.join(REPO, "llm.c-paged_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
