"""CPU tier: the token layer of the device-resident chess loop (csrc/chess_tokens.hip) through its host faces — the same functions the kernels run.

(1) the C ABI of the loop is exported; (2) `lmrl_chess_host_prompt_tokens` == `tokenizer.encode(preprocess_state_og(fen))` with and without left
truncation on every position of tests/golden/chess_perft.json; (3) `lmrl_chess_host_action_from_tokens` == the host path's string work,
`postprocess_move(out_str_process(tokenizer.decode(ids)))` through `VectorChessBoards._strings`' rule, on every SAN of those positions' legal-move
lists and on the corner cases; (4) the reply stream's word is the documented Philox word (restated in oracle/gpt2.py).
Reference: llm_rl_scripts/chess/env/env.py:13-26, 91-143; LLM_RL/algorithms/ppo/gpt2/interface.py:519-546."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from lmrl_gym_amd import _lib
from lmrl_gym_amd.datasets import ByteTokenizer
from lmrl_gym_amd.envs import chess as C

HERE = os.path.dirname(os.path.abspath(__file__))
EOS = 10            # '\n', the eos of an action in the task scripts


def out_str_process(x):
    return x.removesuffix("\n") + "\n"


def strings_rule(s, pitch=C.ACTION_BYTES):
    """VectorChessBoards._strings for one item, as the board reads it: a NUL-terminated string in a fixed-pitch buffer."""
    return s.encode("ascii", errors="replace")[: pitch - 1].split(b"\0")[0]


class CharTokenizer:
    """A character-level tokenizer whose ids are NOT bytes (ids shuffled; two special ids; one multi-character token that is not ASCII)."""
    pad_token_id, eos_token_id = 1, 0
    all_special_ids = [0, 1]

    def __init__(self):
        chars = [chr(c) for c in range(9, 127)]
        random.Random(3).shuffle(chars)
        self.itos = ["<eos>", "<pad>"] + chars + ["é"]
        self.stoi = {c: i for i, c in enumerate(self.itos)}

    def encode(self, s):
        return [self.stoi[c] for c in s]

    def decode(self, ids, skip_special_tokens=False):
        return "".join(self.itos[i] for i in ids if not (skip_special_tokens and i in self.all_special_ids))

    def __len__(self):
        return len(self.itos)


def _ctx(tok, eos, vocab=None, max_new=32):
    from lmrl_gym_amd.chess_rollout import chess_token_tables
    L = _lib.lib()
    vocab = vocab or len(tok)
    byte_id, tb, bl, byte_ids = chess_token_tables(tok, vocab)
    c = L.lmrl_chess_tok_create(byte_id.ctypes.data, tb.ctypes.data, bl.ctypes.data, vocab, 1 if byte_ids else 0, eos, max_new, 8, 1)
    assert c, L.lmrl_last_error()
    return c, byte_ids


def _positions():
    fx = json.load(open(os.path.join(HERE, "golden", "chess_perft.json")))
    return [step["fen"] for game in fx["games"] for step in game["steps"]]


def _legal_sans(fen):
    L = _lib.lib()
    buf = ctypes.create_string_buffer(L.lmrl_chess_pos_bytes())
    assert L.lmrl_chess_host_from_fen(fen.encode(), buf) == 0
    u, s = ctypes.create_string_buffer(256 * 8), ctypes.create_string_buffer(256 * 16)
    k = L.lmrl_chess_host_legal_moves(buf, u, s)
    return [s.raw[i * 16:(i + 1) * 16].split(b"\0")[0].decode() for i in range(k)]


def _action(ctx, ids):
    L = _lib.lib()
    arr = np.asarray(ids, dtype=np.int32)
    out = ctypes.create_string_buffer(C.ACTION_BYTES)
    n = L.lmrl_chess_host_action_from_tokens(ctx, arr.ctypes.data if len(ids) else None, len(ids), out)
    assert n >= 0
    raw = out.raw
    assert raw[n:] == b"\0" * (C.ACTION_BYTES - n) and b"\0" not in raw[:n]
    return raw[:n]


def _expected(tok, ids, eos):
    ids = list(ids)
    if eos in ids:
        ids = ids[: ids.index(eos) + 1]             # generation stops with the eos token (lmrl_gen_accept)
    try:
        text = tok.decode(ids, skip_special_tokens=True)
    except TypeError:
        text = tok.decode([i for i in ids if i != tok.pad_token_id])
    return strings_rule(C.postprocess_move(out_str_process(text)))


def test_chess_token_abi_is_exported():
    L = ctypes.CDLL(_lib.SO_PATH)
    for name in ("lmrl_chess_tok_create", "lmrl_chess_tok_destroy", "lmrl_chess_tok_begin", "lmrl_chess_tok_prompt", "lmrl_chess_tok_action",
                 "lmrl_chess_tok_opponent", "lmrl_chess_tok_opponent_host", "lmrl_chess_tok_result", "lmrl_chess_tok_ppo_records",
                 "lmrl_chess_host_prompt_tokens", "lmrl_chess_host_action_from_tokens", "lmrl_chess_host_reply_word"):
        assert hasattr(L, name), name
        assert name in _lib._SIGS, name


@pytest.mark.parametrize("make_tok", [ByteTokenizer, CharTokenizer])
def test_prompt_tokens_equal_the_tokenizer_on_every_fixture_position(make_tok):
    L = _lib.lib()
    tok = make_tok()
    ctx, _ = _ctx(tok, EOS)
    fens = _positions()
    assert len(fens) > 500
    out = (ctypes.c_int32 * 256)()
    longest = 0
    for fen in fens:
        want = list(tok.encode(C.preprocess_state_og(fen)))
        longest = max(longest, len(want))
        for max_in in (64, 256):
            n = L.lmrl_chess_host_prompt_tokens(ctx, fen.encode(), max_in, out, 256)
            assert list(out[:n]) == want[max(0, len(want) - max_in):], (fen, max_in)         # Truncation.LEFT
    assert longest > 64                                     # the truncated case is exercised
    assert L.lmrl_chess_host_prompt_tokens(ctx, fens[0].encode(), 256, out, 8) == -1
    L.lmrl_chess_tok_destroy(ctx)


def test_tokenizers_that_merge_characters_are_refused():
    from lmrl_gym_amd.chess_rollout import chess_token_tables

    class Merging(ByteTokenizer):
        def encode(self, s):
            return list(s.replace("8 /", "\x01").encode("utf-8"))
    with pytest.raises(ValueError):
        chess_token_tables(Merging(), 257)


def test_action_from_tokens_on_every_legal_san_of_the_fixture():
    tok = ByteTokenizer()
    ctx, byte_ids = _ctx(tok, EOS)
    assert byte_ids
    ctok = CharTokenizer()
    cctx, cbyte = _ctx(ctok, ctok.encode("\n")[0])
    assert not cbyte
    ceos = ctok.encode("\n")[0]
    sans = sorted({s for fen in _positions()[::3] for s in _legal_sans(fen)})
    assert len(sans) > 300
    rng = random.Random(0)
    for san in sans:
        spaced = C.preprocess_move(san)                     # "Q h 5\n"
        for t, c, eos in ((tok, ctx, EOS), (ctok, cctx, ceos)):
            ids = list(t.encode(spaced))
            cases = [ids, ids[:-1], ids + ids, list(t.encode(san)), list(t.encode("  " + spaced + " ")), list(t.encode(spaced[:-1] + "\t\n"))]
            k = rng.randrange(1, len(ids))
            cases.append(ids[:k] + [eos] + ids[k:])                                         # eos in the middle
            cases.append([x for i in ids for x in ([t.pad_token_id, i] if rng.random() < 0.4 else [i])])     # special ids interleaved
            for case in cases:
                got = _action(c, case)
                assert got == _expected(t, case, eos), (san, case)
            assert _action(c, ids) == san.encode()
    L = _lib.lib()
    L.lmrl_chess_tok_destroy(ctx)
    L.lmrl_chess_tok_destroy(cctx)


def test_action_from_tokens_corner_cases():
    tok = ByteTokenizer()
    ctx, _ = _ctx(tok, EOS, max_new=64)
    enc = tok.encode
    cases = [[], [EOS], [256, 256], enc("- -\n"), enc("--"), enc("Z 0\n"), enc("a b c d e f g h i j k l m n o p q r s t\n"), enc("abcdefghijklmnopqrst"),
             enc("abcdefghijklmno"), enc("abcdefghijklmnop"), enc("Q h 5 \t \n"), enc("\n\nQh5"), enc("Q\nh5\n"), enc(" \x0b\x0c\r\x1c\x1d\x1e\x1fe4\x1f "),
             enc("é4\n"), enc("e4é\n"), enc("e 4"), enc(" e4 \n"), enc("　e4"), enc("\x85e4\x85"), enc("\U0001F600e4"),
             [0xC3], [0xC3, 0x28], [0xE2, 0x82], [0xE2, 0x28, 0xA1], [0xE0, 0x80, 0x80], [0xED, 0xA0, 0x80], [0xF0, 0x9F, 0x98], [0xF4, 0x90, 0x80, 0x80],
             [0xF8, 0x88], [0x80, 0xBF, 0x65, 0x34], [0xC0, 0xAF], [0xC3, 256, 0xA9, 0x34], [0xE2, 0x82, 0x65, 0x34, EOS, 0x35],
             [0x65, 0xFF, 0x34, 0xFE], [0xF0, 0x9F, 0x98, 0x80, 0x80], [0xC2, 0x85, 0x65, 0xC2, 0xA0], [0xE1, 0x9A, 0x80, 0x65]]
    rng = random.Random(1)
    for _ in range(3000):                                   # random byte soup around the blanks, newlines and UTF-8 lead / continuation bytes
        n = rng.randrange(0, 24)
        pool = [0x20, 0x0A, 0x09, 0x65, 0x34, 0x51, 0x2D, 0x80, 0xA0, 0x85, 0xBF, 0xC2, 0xC3, 0xE0, 0xE1, 0xE2, 0xED, 0xF0, 0xF4, 0xF5, 0x9A, 0x9F, 256, 0x1F]
        cases.append([rng.choice(pool) if rng.random() < 0.8 else rng.randrange(0, 257) for _ in range(n)])
    for case in cases:
        assert _action(ctx, case) == _expected(tok, case, EOS), case
    assert _action(ctx, enc("- -\n")) == b"--"
    assert _action(ctx, enc("abcdefghijklmnopqrst")) == b"abcdefghijklmno"
    assert _action(ctx, enc("é4\n")) == b"?4"
    # the character tokenizer: a non-ASCII token is one '?', special ids vanish
    ctok = CharTokenizer()
    nl = ctok.encode("\n")[0]
    cctx, _ = _ctx(ctok, nl)
    e_acute = ctok.stoi["é"]
    for case in ([], [nl], [0, 1], ctok.encode("- -\n"), [e_acute] + ctok.encode("4\n"), ctok.encode("e4") + [e_acute, nl], ctok.encode("Q h 5") + [0, nl],
                 ctok.encode("a b c d e f g h i j k l m n o p q r s t\n"), [len(ctok) + 5] + ctok.encode("e4")):
        want = _expected(ctok, [i for i in case if i < len(ctok)], nl) if case and case[0] >= len(ctok) else _expected(ctok, case, nl)
        if case and case[0] >= len(ctok):
            want = b"?" + want                              # an id outside the vocabulary: not text
        assert _action(cctx, case) == want, case
    L = _lib.lib()
    L.lmrl_chess_tok_destroy(ctx)
    L.lmrl_chess_tok_destroy(cctx)


def test_reply_word_is_the_documented_philox_word():
    from oracle.gpt2 import philox4x32_10
    L = _lib.lib()
    rng = random.Random(5)
    for _ in range(200):
        seed, epoch, turn, env = rng.getrandbits(64), rng.getrandbits(32), rng.randrange(0, 4096), rng.randrange(0, 1 << 20)
        want = int(philox4x32_10(env, turn, 0x43484553, epoch, seed & 0xFFFFFFFF, seed >> 32, rounds=7)[0])
        assert L.lmrl_chess_host_reply_word(seed, epoch, turn, env) == want
