"""CPU tier: the text rules of the device-resident Twenty Questions loop (csrc/tq_core.h) through the `lmrl_tq_host_*` faces of csrc/tq_tokens.hip —
the same functions the kernels run — against the Python they replace (lmrl_gym_amd/envs/twenty_questions.py; the reference:
llm_rl_scripts/twenty_questions/env/{env,data,oracle}.py): the question text and its `str.strip()`, the oracle prompt, `answers_from_outputs`,
`is_done` under the stand-in tagger, and the hidden word's draw."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from lmrl_gym_amd import _lib
from lmrl_gym_amd.datasets import ByteTokenizer
from lmrl_gym_amd.envs import twenty_questions as TQ

HERE = os.path.dirname(os.path.abspath(__file__))
EOS = 10                # '\n'
MAX_NEW = 96
PY_SPACES = [chr(c) for c in range(0x110000) if chr(c).isspace()]


def out_str_process(x):
    return x.removesuffix("\n") + "\n"


@pytest.fixture(scope="module")
def rule_tagger():
    TQ.set_pos_tagger(TQ.rule_pos_tag)
    yield
    TQ.set_pos_tagger(None)


@pytest.fixture(scope="module")
def ctx(rule_tagger):
    from lmrl_gym_amd.tq_rollout import tq_context
    words = TQ.get_default_word_list()
    c, info = tq_context(ByteTokenizer(), 260, words, MAX_NEW, 5, EOS, host_only=True)
    yield c, words, info
    _lib.lib().lmrl_tq_destroy(c)


def _question(c, ids):
    L = _lib.lib()
    arr = np.asarray(ids, dtype=np.int32)
    cap = len(ids) + 1
    out = ctypes.create_string_buffer(cap)
    rng = (ctypes.c_int32 * 2)()
    n = L.lmrl_tq_host_question(c, arr.ctypes.data if len(ids) else None, len(ids), out, cap, rng)
    assert 0 < n <= cap
    q = out.raw[:n]
    return q, q[rng[0]:rng[1]]


def _is_done(c, word, question: str):
    raw = question.encode("utf-8")
    j = ctypes.c_int(-1)
    r = _lib.lib().lmrl_tq_host_is_done(c, word, raw, len(raw), ctypes.byref(j))
    assert r in (0, 1) and j.value in (0, 1)
    return bool(r), bool(j.value)


def test_tq_abi_is_exported():
    L = ctypes.CDLL(_lib.SO_PATH)
    for name in ("lmrl_tq_create", "lmrl_tq_destroy", "lmrl_tq_reset", "lmrl_tq_question", "lmrl_tq_oracle_prompt", "lmrl_tq_history_chunk", "lmrl_tq_answer",
                 "lmrl_tq_judge", "lmrl_tq_ppo_records", "lmrl_tq_host_question", "lmrl_tq_host_oracle_prompt", "lmrl_tq_host_answer", "lmrl_tq_host_is_done",
                 "lmrl_tq_host_draw_word"):
        assert hasattr(L, name), name
        assert name in _lib._SIGS, name


def test_question_and_strip_equal_python(ctx):
    """ids -> `out_str_process(tokenizer.decode(ids))` and its `str.strip()`: every Python whitespace code point at either end, invalid UTF-8, the
    empty string, ids that decode to nothing, a missing / doubled final newline, an eos in the middle."""
    c, _, _ = ctx
    tok = ByteTokenizer()
    assert len(PY_SPACES) >= 25 and any(ord(s) > 0x2000 for s in PY_SPACES)
    texts = ["", "\n", "Is it a cat?\n", "Is it a cat?", "Is it a cat?\n\n", " \t Is it a cat? \x0b\x0c\r", "café?\n", "\U0001F600 is it\n", "\u200bx\u200b", "\ufeffx"]
    for s in PY_SPACES:
        texts += [s + "Is it" + s, s + s + "x", "x" + s, s, s + "é" + s + "\n", "a" + s + "b"]
    cases = [list(tok.encode(t)) for t in texts]
    cases += [[0xC3], [0xC3, 0x28], [0xE2, 0x82], [0xE2, 0x28, 0xA1], [0xE0, 0x80, 0x80], [0xED, 0xA0, 0x80], [0xF0, 0x9F, 0x98], [0xF4, 0x90, 0x80, 0x80],
              [0xF8, 0x88], [0x80, 0xBF, 0x65, 0x34], [0xC0, 0xAF], [0xC3, 256, 0xA9, 0x34], [0xE2, 0x82, 0x65, 0x34, EOS, 0x35], [256, 256], [256, EOS],
              [0x20, 0xC2], [0xC2, 0x85, 0x65, 0xC2, 0xA0], [0xE1, 0x9A, 0x80, 0x65, 0xE1, 0x9A], [0xE3, 0x80, 0x80, 0x41, 0xE3, 0x80], [0x41, EOS, 0x42, EOS]]
    rng = random.Random(1)
    pool = [0x20, 0x0A, 0x09, 0x65, 0x3F, 0x80, 0xA0, 0x85, 0xBF, 0xC2, 0xC3, 0xE0, 0xE1, 0xE2, 0xE3, 0xED, 0xF0, 0xF4, 0xF5, 0x9A, 0x9F, 0x81, 0x8A, 0xA8, 0xAF, 256, 0x1F]
    for _ in range(3000):
        cases.append([rng.choice(pool) if rng.random() < 0.85 else rng.randrange(0, 258) for _ in range(rng.randrange(0, 20))])
    for ids in cases:
        cut = ids[: ids.index(EOS) + 1] if EOS in ids else ids         # generation stops with the eos token (lmrl_gen_accept)
        want = out_str_process(tok.decode(cut))
        q, stripped = _question(c, ids)
        assert q == want.encode("utf-8"), ids
        assert stripped == want.strip().encode("utf-8"), ids


def test_oracle_prompt_is_the_env_prompt(ctx):
    c, words, info = ctx
    L = _lib.lib()
    out = (ctypes.c_int32 * 512)()
    for w in (0, 41, 86, len(words) - 1):
        for q in ("Is it a cat?", "", "caf\xe9"):
            raw = q.encode("utf-8")
            n = L.lmrl_tq_host_oracle_prompt(c, w, raw, len(raw), out, 512)
            assert bytes(out[:n]) == TQ.get_oracle_prompt(words[w], q).encode("utf-8")
    assert L.lmrl_tq_host_oracle_prompt(c, 0, b"x", 1, out, 8) == -1
    assert info["prefix_cap"] == max(len(TQ.get_oracle_prompt(w, "").encode()) for w in words) - info["suffix_len"]


def test_answer_parsing_equals_answers_from_outputs(ctx):
    c, _, _ = ctx
    L = _lib.lib()
    tok = ByteTokenizer()
    outs = ["yes", " Yes\n", "no.", "nope", "maybe", "", "YES", "y", "Yes.", " \t\x1fyEs", "\u3000yes", "ye", "n", "No", "\xa0NO", "y\xe9", "\xfdes", "noyes", "\n"]
    questions = ["Is it a cat?"] * len(outs) + [TQ.INVALID_QUESTION, TQ.INVALID_QUESTION, TQ.INVALID_QUESTION.strip()]
    outs = outs + ["yes", "no", "yes"]
    want, _ = TQ.answers_from_outputs(questions, outs)
    assert want[-3:] == ["No.", "No.", "Yes."] and "Yes." in want[:7]
    for q, o, w in zip(questions, outs, want):
        ids = np.asarray(tok.encode(o), dtype=np.int32)
        raw = q.encode("utf-8")
        code = L.lmrl_tq_host_answer(c, raw, len(raw), ids.ctypes.data if len(ids) else None, len(ids))
        assert code in (0, 1) and ("Yes." if code else "No.") == w, (q, o)


def test_judge_equals_is_done_on_the_pinned_questions(ctx):
    c, words, _ = ctx
    fx = json.load(open(os.path.join(HERE, "golden", "twenty_questions.json")))
    assert [w.words for w in words] == fx["word_list"]
    n_true = 0
    for row in fx["is_done"]:
        got, judgeable = _is_done(c, row["word"], row["question"])
        assert judgeable and got == row["done"] == TQ.is_done(words[row["word"]], row["question"]), row
        n_true += got
    assert n_true >= 10 and len(fx["is_done"]) > 300


def _generated_questions(w):
    qs = []
    for sp in w.words:
        low = sp.lower()
        qs += [f"Is it a {low}?", f"Is it {sp}", f"is it the {sp.upper()} ?!  ", f"Is the dinosaur a {low}?", f"Is the dinosaur of {low}?", f"Is it a bucket of {low}?",
               f"Is it a {low}?? 123", f"Is it a {low} 42", f"Is it a {low}...", f"Is it 7 {low}", f"Does the bus have a {low}?", f"Does the buses have a {low}?",
               f"Is it a {low}s?", f"Is it the gas {low}?", f"Is it the glass {low}?", f"Is it the object's {low}?", f"Is it the {low}'s?", f"Is it a '{low}'?",
               f"Is it a {low}\t?\x1f", f"Is it a {low} or something?", f"Is it a kind of {low}", f"is it a {low}, or a type of {low}", f"{low}", f"{low} it is"]
        parts = low.split(" ")
        if len(parts) > 1:
            qs += [f"Is it a {parts[-1]}?", f"Is it a {parts[0]}?", f"Is it a {' '.join(parts[1:])}?", f"Is it a {' '.join(parts[:-1])}?",
                   f"Is it a {parts[0]} big {parts[-1]}?", f"Is it a {parts[-1]} {parts[0]}?"]
    return qs


def test_judge_equals_is_done_on_generated_questions_for_every_word(ctx):
    """Per spelling of every word of the default list: the naming question, a stray noun, a counter noun before `of`, trailing punctuation and digits,
    plural -s of length <= 3 and > 3, apostrophes, multi-word spellings that match only partly."""
    c, words, _ = ctx
    n, n_true, partial = 0, 0, 0
    for wi, w in enumerate(words):
        for q in _generated_questions(w):
            want = TQ.is_done(w, q)
            got, judgeable = _is_done(c, wi, q)
            assert judgeable and got == want, (wi, q, want)
            n += 1
            n_true += want
        other = words[(wi + 7) % len(words)]
        for q in _generated_questions(other)[:6]:
            want = TQ.is_done(w, q)
            assert _is_done(c, wi, q) == (want, True), (wi, q)
        partial += any(len(sp.split(" ")) > 1 for sp in w.words)
    assert n > 3000 and n_true > 500 and n - n_true > 500 and partial > 20
    for q in ("", "?", "12", " ", "'", "of", "a of"):
        assert _is_done(c, 0, q) == (TQ.is_done(words[0], q), True), q


def test_non_ascii_questions_are_not_judged(ctx):
    c, words, _ = ctx
    for q in ("Is it a cat\xa0?", "Is it a c\xe1t?", "Is it a cat? \U0001F600", "\u3000Is it a cat", "Is it a c\xe4t"):
        assert _is_done(c, 10, q) == (False, False), q
    assert TQ.is_done(words[10], "Is it a cat\xa0?") and _is_done(c, 10, "Is it a cat ?") == (True, True)


def test_word_draw_equals_random_choice_and_the_deterministic_mode():
    L = _lib.lib()
    rng = random.Random(4)
    seeds = [0, 1, 2, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1] + [rng.getrandbits(k) for k in range(1, 65) for _ in range(2)]
    n_words = len(TQ.get_default_word_list())
    for n in (n_words, 1, 2, 7, 1000):
        lst = list(range(n))
        for s in seeds:
            assert L.lmrl_tq_host_draw_word(s, 0, n) == random.Random(s).choice(lst), (s, n)
            assert L.lmrl_tq_host_draw_word(s, 1, n) == s % n, (s, n)
    env = TQ.BatchedTwentyQuestionsPolicyEnvironment(None, TQ.get_default_word_list(), bsize=4)
    env.reset([3, 14, 2 ** 40 + 5, 9], [None, dict(deterministic=True), None, dict(deterministic=True)])
    assert [int(i) for i in env._games.word_idx] == [L.lmrl_tq_host_draw_word(3, 0, n_words), L.lmrl_tq_host_draw_word(14, 1, n_words),
                                                     L.lmrl_tq_host_draw_word(2 ** 40 + 5, 0, n_words), L.lmrl_tq_host_draw_word(9, 1, n_words)]


def test_merging_tokenizers_are_refused():
    from lmrl_gym_amd.tq_rollout import tq_context

    class Merging(ByteTokenizer):
        def encode(self, s):
            return list(s.replace("es", "\x01").encode("utf-8"))
    with pytest.raises(ValueError, match="generic"):
        tq_context(Merging(), 260, TQ.get_default_word_list(), 8, 3, EOS, host_only=True)
