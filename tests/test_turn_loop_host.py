"""CPU tier: the host helpers of `lmrl_gym_amd.turn_loop` that the device rollout loops share — generation decoding, the summary dict, the
scripted-steering table and the env seeds of an episode batch.  No GPU and no library load."""
import itertools

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from lmrl_gym_amd.turn_loop import decode_generation, round_seeds, steer_script, summarize

EOS, PAD = 10, 99


class KeywordTokenizer:
    """Accepts `skip_special_tokens` (as a HF tokenizer): ids >= 90 are special."""

    def decode(self, ids, skip_special_tokens=False):
        return "".join("<%d>" % i if i >= 90 else chr(65 + i) for i in ids if not (skip_special_tokens and i >= 90))


class PlainTokenizer:
    """No keyword: `decode(ids, skip_special_tokens=True)` raises TypeError."""
    pad_token_id = PAD

    def decode(self, ids):
        return "".join("<%d>" % i if i >= 90 else chr(65 + i) for i in ids)


class PlainTokenizerWithSpecials(PlainTokenizer):
    all_special_ids = [95, 96]


def test_decode_generation_with_the_keyword():
    assert decode_generation(KeywordTokenizer(), [0, 95, 1, PAD, 2]) == "ABC"


def test_decode_generation_fallback_drops_what_the_tokenizer_declares_special():
    ids = [0, 95, 1, PAD, 2, 96]
    assert decode_generation(PlainTokenizerWithSpecials(), ids) == "AB<99>C"        # all_special_ids: the pad id is not among them and stays
    assert decode_generation(PlainTokenizer(), ids) == "A<95>BC<96>"                # only pad_token_id
    assert decode_generation(PlainTokenizer(), []) == ""


@pytest.mark.parametrize("tok", [KeywordTokenizer(), PlainTokenizer(), PlainTokenizerWithSpecials()])
def test_decode_generation_cuts_behind_the_first_eos_only_when_asked(tok):
    ids = [0, 1, EOS, 2, EOS, 3]
    assert decode_generation(tok, ids) == decode_generation(tok, ids, None) == "ABKCKD"     # an eos id that is not special is ordinary text and stays
    assert decode_generation(tok, ids, EOS) == "ABK"
    assert decode_generation(tok, ids, 42) == "ABKCKD"                                       # an eos that does not occur
    assert ids == [0, 1, EOS, 2, EOS, 3]


def test_steer_script_table():
    import torch
    T, G, B = 3, 4, 5
    rows = [[None] * B for _ in range(T)]
    rows[0][1] = [7, 8]
    rows[1][0] = (1, 2, 3, 4, 5, 6)                     # longer than max_new: cut
    rows[2][4] = []
    steer, counter, cur, strength = steer_script(rows, T, G, B, torch.device("cpu"), 30)
    assert steer.shape == (5 * T + 8, G, B) and steer.dtype == torch.int32
    want = np.full((5 * T + 8, G, B), -1, dtype=np.int32)
    want[0, :2, 1] = [7, 8]
    want[1, :, 0] = [1, 2, 3, 4]
    assert np.array_equal(steer.numpy(), want)          # -1 wherever nothing is scripted: None entries, short ids, the slack rows
    assert counter.shape == (1,) and counter.dtype == torch.int32 and int(counter[0]) == 0
    assert cur.shape == (G, B) and cur.dtype == torch.int32 and bool((cur == -1).all())
    assert strength == 30.0 and isinstance(strength, float)


def test_summarize_passes_dtypes_through():
    f = summarize(np.asarray([1.0, 2.0, 4.0], dtype=np.float32))
    assert f["mean"].dtype == np.float32 and f["min"].dtype == np.float32 and f["max"] == np.float32(4.0)
    assert f == dict(mean=np.mean(np.float32([1, 2, 4])), std=np.std(np.float32([1, 2, 4])), min=np.float32(1), max=np.float32(4))
    i = summarize(np.asarray([3, 1, 2], dtype=np.int64))
    assert i["min"].dtype == np.int64 and i["max"].dtype == np.int64 and i["mean"].dtype == np.float64 and i["mean"] == 2.0
    assert summarize([2, 2])["std"] == 0.0              # plain lists too (`text_env_eval`'s lengths)
    assert sorted(f) == ["max", "mean", "min", "std"]


@pytest.mark.parametrize("draw", [True, False])
def test_round_seeds_consume_exactly_the_live_envs_values(draw):
    gen = itertools.count(100)
    assert round_seeds(8, 3, gen, draw) == [100, 101, 102, 0, 0, 0, 0, 0]
    assert next(gen) == 103                             # exactly `actual` values were taken
    assert round_seeds(4, 4, gen, draw) == [104, 105, 106, 107]
    assert round_seeds(4, 0, gen, draw) == [0, 0, 0, 0] and next(gen) == 108


def test_round_seeds_without_a_generator():
    assert round_seeds(6, 4, None, draw=False) == [0] * 6
    state = np.random.get_state()
    try:
        np.random.seed(5)
        got = round_seeds(6, 4, None)
        np.random.seed(5)
        want = np.random.randint(0, 2 ** 31 - 1, size=4).tolist()       # ONE draw of `actual` values from numpy's global stream
        after = np.random.randint(0, 1000)
        np.random.seed(5)
        round_seeds(6, 4, None)
        assert np.random.randint(0, 1000) == after
    finally:
        np.random.set_state(state)
    assert got == want + [0, 0] and all(isinstance(s, int) for s in got)


def test_engine_round_seeds_follow_the_engines_rule():
    from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
    from lmrl_gym_amd.maze_rollout import MazeRolloutEngine
    from lmrl_gym_amd.tq_rollout import TwentyQuestionsRolloutEngine
    from lmrl_gym_amd.turn_loop import TurnLoopEngine
    for cls, draws in ((MazeRolloutEngine, True), (TwentyQuestionsRolloutEngine, True), (ChessRolloutEngine, False)):
        assert issubclass(cls, TurnLoopEngine)
        eng = cls.__new__(cls)                          # the seed rule needs nothing but B
        eng.B = 5
        gen = itertools.count(7)
        assert eng._round_seeds(2, gen) == [7, 8, 0, 0, 0] and next(gen) == 9
        state = np.random.get_state()
        try:
            np.random.seed(11)
            got = eng._round_seeds(3, None)
            np.random.seed(11)
            want = np.random.randint(0, 2 ** 31 - 1, size=3).tolist() if draws else [0, 0, 0]
        finally:
            np.random.set_state(state)
        assert got == want + [0, 0]
