"""logit_ref64 (the float64 restatement of the logit processors) on
hand-computed cases, and the soundness of the kernel test's exact-id
assertion: for its fixed inputs every row's reference winner leads the best
other column by more than 2 tol, or ties it exactly."""
import numpy as np
import pytest

import logit_ref64 as lr


def _row(vals):
    return np.array(vals, np.float32)


def test_repetition_rule_and_its_sign_branch():
    x = _row([2.0, -2.0, 0.0, 3.0, -1.0])
    c = np.array([1, 2, 1, 0, 0])
    y, tol = lr.process(x, c, r=2.0)
    assert y.tolist() == [1.0, -4.0, 0.0, 3.0, -1.0]  # positive divided, negative (and zero) multiplied, unseen kept
    assert tol.tolist() == [2.0 ** -21 * v for v in (1.0, 4.0, 0.0, 3.0, 1.0)]


def test_presence_alone():
    y, tol = lr.process(_row([1.0, 1.0, -1.0]), np.array([0, 1, 5]), p=0.5)
    assert y.tolist() == [1.0, 0.5, -1.5]  # once per seen token, however often
    assert tol.tolist() == [2.0 ** -21 * v for v in (1.0, 1.5, 1.5)]


def test_frequency_alone():
    y, _ = lr.process(_row([1.0, 1.0, -1.0]), np.array([0, 1, 4]), f=0.25)
    assert y.tolist() == [1.0, 0.75, -2.0]


def test_order_of_the_rules():
    # (4 / 2) - 0.5 * 3 - 0.25 + 1 = 1.25; a negative logit: (-4 * 2) - 1.5 - 0.25 = -9.75
    y, tol = lr.process(_row([4.0, -4.0]), np.array([3, 3]), r=2.0, p=0.25, f=0.5, bias_ids=[0], bias_vals=[1.0])
    assert y.tolist() == [1.25, -9.75]
    assert tol.tolist() == [2.0 ** -21 * (2.0 + 1.5 + 0.25 + 1.0), 2.0 ** -21 * (8.0 + 1.5 + 0.25)]


def test_neutral_settings_return_the_input_bits():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(500) * 5).astype(np.float32)
    x[:3] = (0.0, -0.0, np.float32(1e-42))  # zeros of both signs, a subnormal
    c = rng.integers(0, 4, 500)
    y, _ = lr.process(x, c)
    assert y.astype(np.float32).tobytes() == x.tobytes()


def test_a_ban_and_a_finite_bias():
    x = _row([1.0, 5.0, 2.0])
    y, tol = lr.process(x, np.zeros(3, int), bias_ids=[1, 2], bias_vals=[-np.inf, 0.5])
    assert y[0] == 1.0 and np.isneginf(y[1]) and y[2] == 2.5
    assert np.isfinite(tol).all()
    assert lr.winner(y) == 2
    lr.assert_close(np.array([1.0, -np.inf, 2.5], np.float32), y, tol)
    with pytest.raises(AssertionError):
        lr.assert_close(np.array([1.0, -1e30, 2.5], np.float32), y, tol)  # a ban is -inf, not a large negative
    with pytest.raises(AssertionError):
        lr.assert_close(np.array([1.0, -np.inf, 2.5001], np.float32), y, tol)


def test_the_window_from_pos():
    hist = [7, 7, 3, 9, 7, 3]
    assert lr.counts_from(hist, 0, 6, 10).tolist() == [0, 0, 0, 2, 0, 0, 0, 3, 0, 1]
    assert lr.counts_from(hist, 2, 6, 10).tolist() == [0, 0, 0, 2, 0, 0, 0, 1, 0, 1]  # the prompt's two 7s left out
    assert lr.counts_from(hist, 2, 4, 10).tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1]  # ... and what lies past pos
    assert lr.counts_from(hist, 6, 6, 10).sum() == 0 and lr.counts_from(hist, 9, 6, 10).sum() == 0


def test_winner_rules():
    assert lr.winner(np.array([1.0, 3.0, 3.0])) == 1  # lowest index on ties
    assert lr.winner(np.full(4, -np.inf)) == 0  # nothing above -inf
    w, gap, bar = lr.lead(np.array([-np.inf, 2.0, -np.inf]), np.zeros(3))
    assert (w, gap, bar) == (1, np.inf, 0.0)


@pytest.mark.parametrize("V,kinds", lr.KERNEL_CASES)
def test_kernel_inputs_have_clear_or_exactly_tied_winners(V, kinds):
    case = lr.kernel_case(V, kinds)
    assert case["counts"].max() <= 1000 and case["bias_n"].max() <= lr.BIAS_MAX
    for b, (y, tol) in enumerate(lr.kernel_reference(case)):
        kind = kinds[b]
        n = int(case["bias_n"][b])
        assert len(set(case["bias_ids"][b, :n].tolist())) == n  # distinct ids
        w, gap, bar = lr.lead(y, tol)
        assert gap == 0.0 or gap > bar, (V, b, kind, w, gap, bar)
        if kind == lr.NEUTRAL:  # the planted tie: both columns hold the row maximum, the lower one wins
            assert gap == 0.0 and y.astype(np.float32).tobytes() == case["x"][b].tobytes()
        if kind == lr.REPETITION:
            top = int(np.argmax(case["x"][b]))
            assert case["counts"][b, top] > 0 and (case["x"][b] > 0).any() and (case["x"][b] < 0).any()
        if kind == lr.PRES_FREQ:
            cc = case["counts"][b]
            assert cc[cc > 0].min() == 1 and cc.max() == 1000
        if kind == lr.BIAS_LAST:
            assert w == V - 1 and np.isneginf(y[int(np.argmax(case["x"][b]))])
        if kind == lr.BIAS_FIRST:
            assert w == 0 and np.isneginf(y[int(np.argmax(case["x"][b]))])
        if kind == lr.ALL_BUT_ONE:
            assert np.isfinite(y).sum() == 1 and w == int(np.flatnonzero(np.isfinite(y))[0]) and w != 0
        if kind == lr.ALL_BANNED:
            assert not np.isfinite(y).any() and w == 0
