"""CPU tier: the beam-search oracle (tests/beam_oracle.py, the numpy float64 restatement of the rules in DESIGN.md "Beam search") against brute
force, a hand-worked case and hand-computed stopping steps.  The GPU tests hold the kernels to this oracle."""
import itertools
import math

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
import beam_oracle as BO


def _table_fn(table):
    """logits_fn over a dict {generated prefix (tuple) -> logits [V]}; beams that were never alive carry arbitrary prefixes of the same length."""
    return lambda seqs: np.stack([table[tuple(s)] for s in seqs])


@pytest.mark.parametrize("seed", range(8))
def test_exhaustive_width_finds_the_brute_force_optimum(seed):
    """V = 6, 3 new tokens, K = 36 = V ** 2 beams, length_penalty = 0 (scores are plain sums of log-probabilities), all three positions run
    (stop_rule=False: with K > V most running beams were never alive, and the loop condition, which reads the LAST running beam, would end the
    search after the first position — the stopping rule has its own test below).  No live hypothesis is ever cut (<= 25 live beams, all 6
    continuations of each among the top 2K = 72 unless 72 better ones exist), so the finished pool's best entry is the best eos-terminated
    sequence and the first running beam the best full-length one.  The rules return the finished one whenever one exists (here always): where the
    brute-force optimum over eos-terminated AND full-length sequences ends in eos, the returned sequence is that optimum."""
    V, T, K, eos = 6, 3, 36, 5
    rng = np.random.RandomState(seed)
    table = {p: rng.randn(V) * 2.0 for n in range(T) for p in itertools.product(range(V), repeat=n)}
    lsm = {p: BO.log_softmax(v) for p, v in table.items()}
    finished, full = {}, {}
    for n in range(1, T + 1):
        for p in itertools.product(range(V), repeat=n):
            if eos in p[:-1]:
                continue
            score = sum(lsm[p[:i]][p[i]] for i in range(n))
            if p[-1] == eos:
                finished[p] = score
            elif n == T:
                full[p] = score
    last = {}
    seqs, scores, steps, _ = BO.beam_search(_table_fn(table), 1, K, 7, T, eos, length_penalty=0.0, stop_rule=False,
                                            on_step=lambda t, a, info, b: last.update(st=b))
    assert steps == T
    best_fin = max(finished, key=finished.get)
    best_full = max(full, key=full.get)
    assert tuple(seqs[0]) == best_fin and scores[0] == pytest.approx(finished[best_fin], abs=1e-9)
    assert tuple(last["st"].run_seq[0][0]) == best_full and last["st"].run_score[0][0] == pytest.approx(full[best_full], abs=1e-9)
    everything = {**finished, **full}
    best = max(everything, key=everything.get)
    if best[-1] == eos:
        assert tuple(seqs[0]) == best


# ---- hand-worked: K = 2, V = 4, eos = 3, length_penalty = 0 (pool scores are sums of log-probabilities).  Probabilities per generated prefix:
_P = {(): [.5, .3, .12, .08],
      (0,): [.4, .06, .04, .5], (1,): [.6, .06, .04, .3],
      (0, 0): [.7, .2, .06, .04], (1, 0): [.05, .03, .02, .9],
      (0, 0, 0): [.25] * 4, (0, 0, 1): [.25] * 4}


def _hand_fn(seqs):
    # beam 1 of position 0 was never alive (score -1e7): it stands on the empty prefix like beam 0
    return np.log(np.array([_P[tuple(s)] for s in seqs]))


def test_hand_worked_two_beams_three_steps_with_a_displaced_eos():
    """Position 0: candidates .5 (0), .3 (1), .12 (2), .08 (eos) -> running [0], [1]; pool: [eos] at ln .08.
    Position 1: products .25 (0 eos), .20 (0 0), .18 (1 0), .09 (1 eos) -> running [0 0] from beam 0, [1 0] from beam 1; pool: [0 eos] ln .25,
    [1 eos] ln .09 — the [eos] of position 0 (ln .08) is displaced.
    Position 2: .162 (1 0 eos), .14 (0 0 0), .04 (0 0 1), .012 (0 0 2) -> running [0 0 0], [0 0 1], both from beam 0; pool: [0 eos] ln .25,
    [1 0 eos] ln .162 — [1 eos] is displaced too."""
    log = []
    seqs, scores, steps, _ = BO.beam_search(_hand_fn, 1, 2, 5, 3, 3, length_penalty=0.0, on_step=lambda t, a, info, b: log.append((info[0], b)))
    assert steps == 3
    (i0, s0), (i1, s1), (i2, s2) = log
    assert i0["cand_tok"].tolist() == [0, 1, 2, 3] and i0["parent"].tolist() == [0, 0] and i0["tok"].tolist() == [0, 1]
    assert s0.fin_seq[0][0] == [3] and s0.fin_flag[0].tolist() == [True, False]
    assert s0.fin_score[0][0] == pytest.approx(math.log(.08)) and s0.fin_score[0][1] == BO.NEG
    assert i1["cand_beam"].tolist() == [0, 0, 1, 1] and i1["cand_tok"].tolist() == [3, 0, 0, 3]
    assert i1["parent"].tolist() == [0, 1] and s1.run_seq[0] == [[0, 0], [1, 0]]
    assert s1.run_score[0].tolist() == pytest.approx([math.log(.20), math.log(.18)])
    assert s1.fin_seq[0] == [[0, 3], [1, 3]] and s1.fin_flag[0].all()
    assert s1.fin_score[0].tolist() == pytest.approx([math.log(.25), math.log(.09)])
    assert i2["parent"].tolist() == [0, 0] and s2.run_seq[0] == [[0, 0, 0], [0, 0, 1]]
    assert s2.run_score[0].tolist() == pytest.approx([math.log(.14), math.log(.04)])
    assert s2.fin_seq[0] == [[0, 3], [1, 0, 3]] and s2.fin_score[0].tolist() == pytest.approx([math.log(.25), math.log(.162)])
    assert seqs == [[0, 3]] and scores[0] == pytest.approx(math.log(.25))


def test_stop_conditions_fire_at_the_hand_computed_step():
    """The case above with room for 4 tokens.  Before position 2 the pool is full ([0 eos], [1 eos]): early_stopping ends the search there, after 2
    positions.  Without it, worst_finished = ln .09 lies below the last running beam (ln .18): position 2 runs; before position 3 worst_finished =
    ln .162 is above the last running beam (ln .04): no improvement is possible and the search ends after 3 positions, not 4."""
    for early, want_steps, want_pool in ((True, 2, [[0, 3], [1, 3]]), (False, 3, [[0, 3], [1, 0, 3]])):
        last = {}
        seqs, scores, steps, _ = BO.beam_search(_hand_fn, 1, 2, 5, 4, 3, length_penalty=0.0, early_stopping=early,
                                                on_step=lambda t, a, info, b: last.update(st=b))
        assert steps == want_steps and last["st"].fin_seq[0] == want_pool
        assert seqs == [[0, 3]] and scores[0] == pytest.approx(math.log(.25))
    # the condition itself, on hand-made states: the LAST running beam decides (BEST_RUNNING_BEAM), and an unflagged pool entry keeps an item open
    st = BO.State(2, 2)
    st.run_score[:] = [[-1.0, -3.0], [-1.0, -3.0]]
    st.fin_flag[:] = True
    st.fin_score[:] = [[-0.5, -2.0], [-0.5, -2.0]]
    assert not BO.keep_going(st, 1, 4, 6, 0.0, False)            # -2 is not below -3, in either item
    st.fin_score[1, 1] = -3.5
    assert BO.keep_going(st, 1, 4, 6, 0.0, False)                # one item of the batch keeps the loop alive
    assert not BO.keep_going(st, 1, 4, 6, 0.0, True)             # every pool full: early stopping ends it
    assert not BO.keep_going(st, 4, 4, 6, 0.0, False)            # max_new_tokens
    st.fin_flag[0, 1] = False
    assert BO.keep_going(st, 1, 4, 6, 0.0, True)
    # length_penalty divides the running score by max_length ** length_penalty = 10: -3 / 10 = -0.3 is above -0.5 ... -3.5
    st.fin_flag[:] = True
    st.fin_score[:] = [[-0.2, -0.25], [-0.2, -0.25]]
    assert BO.keep_going(st, 1, 4, 6, 0.0, False) is False and BO.keep_going(st, 1, 4, 6, 1.0, False) is False
    st.fin_score[0, 1] = -0.4
    assert BO.keep_going(st, 1, 4, 6, 1.0, False) and not BO.keep_going(st, 1, 4, 6, 0.0, False)
