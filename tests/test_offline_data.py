"""CPU tier of the device offline-data build (csrc/offline_data.hip, algorithms/offline_device.py) against
tests/golden/offline_rl_data.json, which tests/golden/make_offline_data_fixture.py produced by running the reference's
`TokenTrajectoryChain.from_text_trajectory_chain`, `ILQLData.from_token_trajectory_chain` and `MCData.from_token_trajectory_chain`.
No GPU: the token layer runs through its host face, the block rule as an index-form numpy restatement of the kernel."""
import ctypes

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from conftest import load_golden
from lmrl_gym_amd import _lib
from lmrl_gym_amd import environment as E
from lmrl_gym_amd.algorithms import bc
from lmrl_gym_amd.algorithms import offline_device as OD
from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
from lmrl_gym_amd.algorithms.ilql import ILQLData
from lmrl_gym_amd.algorithms.mc_returns import MCData
from lmrl_gym_amd.datasets import MaskDataset, WordleTokenizer
from lmrl_gym_amd.envs import wordle as W
from lmrl_gym_amd.envs import wordle_policies as P
from lmrl_gym_amd.rollout import WordleTokenTable

G = load_golden("offline_rl_data.json")
CAP = 76          # header (4) + 6 turns x (6 action + 6 observation tokens)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_record(ep, table=None, cap=CAP):
    """One fixture episode through lmrl_wordle_host_scripted_record -> (tokens, is_action, reward [cap], n_tok, done)."""
    table = table or WordleTokenTable.default_gpt2()
    k = len(ep["actions"])
    guess, obs = np.zeros(6, np.uint32), np.zeros(6, np.uint32)
    reward, flags = np.zeros(6, np.float32), np.zeros(6, np.uint8)
    for t in range(k):
        guess[t], obs[t], reward[t] = W.pack_guess(ep["actions"][t]), P.obs_code(ep["observations"][t]), ep["rewards"][t]
    flags[k - 1] = 1 if ep["done"] else 0
    tok, ia, rw = np.full(cap, -7, np.int32), np.full(cap, 9, np.uint8), np.full(cap, np.nan, np.float32)
    done = ctypes.c_int(-1)
    ct = table.c_struct()
    n = _lib.lib().lmrl_wordle_host_scripted_record(ctypes.byref(ct), _ptr(guess), _ptr(obs), _ptr(reward), _ptr(flags), k, cap, _ptr(tok), _ptr(ia),
                                                    _ptr(rw), ctypes.byref(done))
    return tok, ia, rw, n, done.value


def test_fixture_covers_every_length_and_a_bad_word():
    assert {len(e["actions"]) for e in G["episodes"]} == {1, 2, 3, 4, 5, 6}
    bad = [e for e in G["episodes"] if e["bad_word"]]
    assert bad and any(o == "" for e in bad for o in e["observations"])
    nexts = [l["ilql"] for c in G["chains"] for l in c["links"]]
    assert any(x["next_token_ids"] is not None and x["next_done"] for x in nexts)                    # a next trajectory without any action, done
    assert any(x["next_token_ids"] is not None and len(x["next_token_ids"]) == 1 for x in nexts)      # first action of the next at index 1


def test_host_face_equals_the_reference_tokens_on_every_episode():
    table = WordleTokenTable.default_gpt2()
    for ep in G["episodes"]:
        tok, ia, rw, n, done = host_record(ep, table)
        assert n == len(ep["tokens"]), (ep["case"], ep["index"])
        assert tok[:n].tolist() == ep["tokens"]
        assert ia[:n].tolist() == ep["is_action"]
        assert (rw[:n].view(np.uint32) == np.asarray(ep["reward"], np.float32).view(np.uint32)).all()
        assert done == int(ep["done"])
        assert (tok[n:] == table.pad).all() and not ia[n:].any() and not rw[n:].any()      # the rest of the row: pad / 0 / 0
    # an episode that does not fit the row is refused, not cut
    ep = max(G["episodes"], key=lambda e: len(e["tokens"]))
    assert host_record(ep, table, cap=len(ep["tokens"]) - 1)[3] == -1
    assert host_record(ep, table, cap=len(ep["tokens"]))[3] == len(ep["tokens"])


def test_host_face_follows_the_token_table():
    """Other ids, a longer header: the rows are `WordleTokenizer(table).encode` of the reformatted texts."""
    base = WordleTokenTable.default_gpt2()
    table = WordleTokenTable(newline=7, pad=3, letter_first=[100 + i for i in range(26)], letter_sp=[200 + i for i in range(26)],
                             sym_first=[106, 124, 101], sym_sp=[206, 224, 201], header=[11, 12, 13, 14, 7])
    assert len(base.header) == 4
    tk = WordleTokenizer(table)
    for ep in G["episodes"][:8]:
        raw = tuple()
        for a, o in zip(ep["actions"], ep["observations"]):
            raw += (E.Text(a, True), E.Text(o, False))
        want = [table.header] + [tk.encode(t.text) for t in W.reformat_history(raw)[1:]]
        tok, ia, rw, n, _ = host_record(ep, table, cap=80)
        assert tok[:n].tolist() == sum(want, [])


# ------------------------------------------------------------------------------------------------ the block rule
def np_block(rows, T, pad, left, returns=None):
    """The index form `offline_block_kernel` implements, restated with numpy.  rows: [(tokens, is_action, reward) full arrays]."""
    m = len(rows)
    out = dict(input_ids=np.full((m, T), pad, np.int32), should_take_action=np.zeros((m, T - 1), np.bool_), rewards=np.zeros((m, T - 1), np.float32),
               returns=np.zeros((m, T - 1), np.float32), training_mask=np.zeros((m, T), np.float32), lengths=np.zeros(m, np.int32))
    for j, (tok, ia, rw) in enumerate(rows):
        nn = len(tok)
        length, off = min(nn, T), (nn - T if left and nn > T else 0)
        for t in range(length):
            out["input_ids"][j, t] = tok[off + t]
            out["training_mask"][j, t] = 1.0 if ia[off + t] else 0.0
        n1 = max(nn - 1, 0)
        len1, off1 = min(n1, T - 1), (n1 - (T - 1) if left and n1 > T - 1 else 0)
        for t in range(len1):
            out["should_take_action"][j, t] = bool(ia[1 + off1 + t])
            out["rewards"][j, t] = rw[1 + off1 + t]
            if returns is not None:
                out["returns"][j, t] = returns[j][off1 + t]
        out["lengths"][j] = length
    return out


def np_next(links, k, T, pad, left):
    """next_token_ids row / next_done of link k of a chain, by the kernel's rule."""
    row = np.full(T, pad, np.int32)
    if k + 1 >= len(links):
        return row, True                                   # the chain's last trajectory: all padding, no bootstrap
    nx = links[k + 1]
    ia, tok = nx["is_action"], nx["tokens"]
    first = next((t for t in range(1, len(tok)) if ia[t]), -1)
    seq, nd = (tok[:first], False) if first >= 0 else (tok, bool(nx["done"]))
    kept, off = min(len(seq), T), (len(seq) - T if left and len(seq) > T else 0)
    row[:kept] = seq[off:off + kept]
    return row, nd


class _Tok:
    pad_token_id = G["pad_token_id"]


CUTS = [8, 13, 128]        # RIGHT: inside the first action (tokens 4-9), inside the first observation (10-15), no truncation


@pytest.mark.parametrize("trunc", [Truncation.RIGHT, Truncation.LEFT])
@pytest.mark.parametrize("T", CUTS)
def test_block_rule_equals_the_host_forms(trunc, T):
    eps = G["episodes"]
    left = trunc == Truncation.LEFT
    bs = BlockingStrategy(Padding.RIGHT, trunc, T)
    rows = [(e["tokens"], e["is_action"], e["reward"]) for e in eps]
    got = np_block(rows, T, _Tok.pad_token_id, left, returns=[e["mc"]["returns"] for e in eps])
    arr = lambda x, dt: np.asarray(x, dtype=dt)
    il = ILQLData.block([ILQLData(arr(e["tokens"], np.int32), arr(e["ilql"]["should_take_action"], np.bool_), arr(e["ilql"]["rewards"], np.float32),
                                  e["ilql"]["done"], None, None) for e in eps], bs, _Tok)
    assert (got["input_ids"] == il["input_ids"]).all() and (got["should_take_action"] == il["should_take_action"]).all()
    assert (got["rewards"].view(np.uint32) == il["rewards"].view(np.uint32)).all()
    assert il["next_token_ids"] is None
    mc = MCData.block([MCData(arr(e["tokens"], np.int32), arr(e["mc"]["should_take_action"], np.bool_), arr(e["mc"]["returns"], np.float32)) for e in eps],
                      bs, _Tok)
    assert (got["input_ids"] == mc["input_ids"]).all() and (got["should_take_action"] == mc["should_take_action"]).all()
    assert (got["returns"].view(np.uint32) == mc["returns"].view(np.uint32)).all()
    segs = []
    for e in eps:
        raw = tuple()
        for a, o in zip(e["actions"], e["observations"]):
            raw += (E.Text(a, True), E.Text(o, False))
        segs.append([(t.text, float(t.is_action)) for t in W.reformat_history(raw)])
    md = MaskDataset.blocked_from_str_segments(segs, WordleTokenizer(), bs)
    assert (got["input_ids"] == md.input_ids).all() and (got["training_mask"] == md.input_training_mask).all()
    assert (got["lengths"] == np.minimum([len(e["tokens"]) for e in eps], T)).all()
    if T < 128:      # the cut really lands where the case says, on some episode
        cut_at = [(len(e["tokens"]) - T if left else T) for e in eps if len(e["tokens"]) > T]
        kinds = {bool(e["is_action"][c]) for e, c in zip([e for e in eps if len(e["tokens"]) > T], cut_at)}
        # RIGHT: the first dropped token is token T — inside the first action for 8, inside the first observation for 13 (a bad-word episode's
        # one-token observation aside); LEFT: the first kept token sits T tokens before the end — inside the last action for 8 (six observation
        # tokens + two action tokens), inside an observation (or the header) for 13
        assert (T == 8) in kinds


@pytest.mark.parametrize("trunc", [Truncation.RIGHT, Truncation.LEFT])
@pytest.mark.parametrize("T", [5, 9, 64])
def test_chain_rule_equals_the_reference_items(trunc, T):
    left = trunc == Truncation.LEFT
    bs = BlockingStrategy(Padding.RIGHT, trunc, T)
    pad = _Tok.pad_token_id
    arr = lambda x, dt: np.asarray(x, dtype=dt)
    for c in G["chains"]:
        links = c["links"]
        for k, l in enumerate(links):
            row, nd = np_next(links, k, T, pad, left)
            ref = l["ilql"]
            if ref["next_token_ids"] is None:
                assert k == len(links) - 1 and nd and (row == pad).all()
                continue
            il = ILQLData.block([ILQLData(arr(l["tokens"], np.int32), arr(ref["should_take_action"], np.bool_), arr(ref["rewards"], np.float32), ref["done"],
                                          arr(ref["next_token_ids"], np.int32), ref["next_done"])], bs, _Tok)
            assert (row == il["next_token_ids"][0]).all() and nd == bool(il["next_dones"][0])
            got = np_block([(l["tokens"], l["is_action"], l["reward"])], T, pad, left)
            assert (got["input_ids"] == il["input_ids"]).all() and (got["should_take_action"] == il["should_take_action"]).all()
            assert (got["rewards"].view(np.uint32) == il["rewards"].view(np.uint32)).all()
            assert bool(il["dones"][0]) == (k == len(links) - 1 and l["done"])


def test_only_right_padding_is_built():
    with pytest.raises(ValueError):
        OD._strategy(BlockingStrategy(Padding.LEFT, Truncation.RIGHT, 16), None)
    with pytest.raises(ValueError):
        OD._strategy(BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 1), None)
    assert OD._strategy(BlockingStrategy(Padding.RIGHT, Truncation.LEFT, 16), None) == (16, True)
    assert OD._strategy(BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 16), None) == (16, False)


# ------------------------------------------------------------------------------------------------ the filter
SCORES = [np.array([-6.0, -3.0, -3.0, -1.0, -3.0, -6.0, 0.0, -2.0, -3.0, -5.0]),            # ties across the cut
          np.array([-1.0] * 7), np.array([0.0, -1.0, -2.0, -3.0]),
          np.random.default_rng(5).integers(-6, 1, size=101).astype(np.float64)]


@pytest.mark.parametrize("scores", SCORES, ids=["ties", "all_equal", "sorted", "random101"])
def test_filter_decision_equals_the_host_rules(scores):
    items = list(range(len(scores)))
    for take_top in (10, 30, 50, 100):
        want = bc.filter_items(lambda i: scores[i], items, take_top=take_top)
        assert OD.filter_decision(scores.astype(np.float32), take_top=take_top).tolist() == want
    for thr in (-3.0, -0.5, 1.0):
        want = bc.filter_items(lambda i: scores[i], items, threshold=thr)
        assert OD.filter_decision(scores.astype(np.float32), threshold=thr).tolist() == want
    for frac in (0.0, 0.3, 0.5, 1.0):      # scripts/harness.py filtered-bc: stable sort by reward, descending, then the first int(n * frac)
        want = sorted(range(len(scores)), key=lambda i: scores[i], reverse=True)[: int(len(scores) * frac)]
        assert OD.filter_decision(scores.astype(np.float32), top_fraction=frac).tolist() == want
    with pytest.raises(ValueError):
        OD.filter_decision(scores, take_top=10, threshold=0.0)
    with pytest.raises(ValueError):
        OD.filter_decision(scores)
