"""GPU tier: the device-resident chess rollout loop (`lmrl_gym_amd.chess_rollout.ChessRolloutEngine`, csrc/chess_tokens.hip) against the env and the
generic text path it replaces (`VectorChessEnv` + `GPT2PPOPolicy` + `interact_environment`), its device opponent against the documented reply stream,
and its PPO records against the online script's chains (llm_rl_scripts/chess/ppo/train_ppo_gpt2_online.py:201-340, chess/env/env.py:91-342)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ILLEGAL, MOVED, GAME_OVER, NULL_MOVE = 0, 1, 2, 3
MATE_IN_ONE = "7k/5Q2/6K1/8/8/8/8/8 w - - 0 1"
STALEMATING = "k7/8/8/8/8/8/1Q6/7K w - - 0 1"           # Qb6 leaves black without a move and not in check
HANGING = "8/8/8/8/8/1k6/8/Q6K w - - 0 1"               # Qa2+ hangs the queen: the scripted reply Kxa2 leaves bare kings
TWO_ROOKS = "R6R/8/8/8/8/8/4K3/6k1 w - - 0 1"           # Rd8 is ambiguous, Rad8 is not


class Board:
    """One position on the host faces of the rules (csrc/chess_rules.h)."""

    def __init__(self, fen):
        from lmrl_gym_amd import _lib
        self.L = _lib.lib()
        self.buf = ctypes.create_string_buffer(self.L.lmrl_chess_pos_bytes())
        assert self.L.lmrl_chess_host_from_fen(fen.encode(), self.buf) == 0, fen

    def fen(self):
        out = ctypes.create_string_buffer(96)
        n = self.L.lmrl_chess_host_fen(self.buf, out)
        return out.raw[:n].decode()

    def legal(self):
        u, s = ctypes.create_string_buffer(256 * 8), ctypes.create_string_buffer(256 * 16)
        k = self.L.lmrl_chess_host_legal_moves(self.buf, u, s)
        g = lambda b, i, w: b.raw[i * w:(i + 1) * w].split(b"\0")[0].decode()
        return [(g(u, i, 8), g(s, i, 16)) for i in range(k)]

    def agent(self, san):
        r, d = ctypes.c_float(), ctypes.c_int()
        res = self.L.lmrl_chess_host_agent_step(self.buf, san.encode(), ctypes.byref(r), ctypes.byref(d))
        return res, r.value, bool(d.value)

    def opponent(self, uci):
        r, d, s = ctypes.c_float(), ctypes.c_int(), ctypes.create_string_buffer(16)
        ok = self.L.lmrl_chess_host_opponent_step(self.buf, uci.encode(), s, ctypes.byref(r), ctypes.byref(d))
        assert ok, uci
        return s.value.decode(), r.value, bool(d.value)


def host_game(start, actions, reply_idx, max_moves):
    """FenChessHistoryEnv on the host rules: -> [(fen before, action, result, reward, done, opponent SAN or None, fen after)]."""
    b, out = Board(start), []
    fen = start
    for t, a in enumerate(actions):
        res, r, d = b.agent(a)
        opp = None
        if res == MOVED:
            lm = b.legal()
            opp, r, d = b.opponent(lm[reply_idx[t] % len(lm)][0])
        after = b.fen()
        d = d or t + 1 > max_moves
        out.append((fen, a, res, r, d, opp, after))
        fen = after
        if d:
            break
    return out


class ScriptedPool:
    """An engine object for VectorChessEnv: game `asking[k]` is answered with legal move reply_idx[turn][env] mod count in the host rules' order."""

    def __init__(self, reply_idx):
        self.reply_idx, self.turn, self.asking = reply_idx, 0, []

    def best_moves(self, games):
        assert len(games) == len(self.asking), (len(games), self.asking)
        out = []
        for (start, moves), env in zip(games, self.asking):
            b = Board(start)
            for mv in moves:
                b.opponent(mv)
            lm = b.legal()
            out.append(lm[int(self.reply_idx[self.turn][env]) % len(lm)][0])
        return out

    def close(self):
        pass


def _weights(width, vocab, seed=0, bias_chars="abcdefgh12345678NBRQKxO-=+#\n ", boost=0.5):
    """Random GPT-2 weights whose final layer norm leans towards the SAN alphabet (tied LM head: logit_c += wte_c . bias = about `boost` for the
    alphabet's ids — the size of the context-dependent part of a random model's logits, std 0.02 sqrt(d)), so that greedy decoding spells strings
    from that alphabet that depend on the position."""
    import torch
    from lmrl_gym_amd.gpt2 import GPT2Config, init_hf_style_state_dict
    cfg = GPT2Config(2, 2, 128, 256, vocab, 256) if width == "tiny" else GPT2Config.gpt2_small(vocab)
    sd = init_hf_style_state_dict(cfg, seed=seed)
    if boost:
        sd["ln_f.bias"] = boost / (cfg.initializer_range ** 2 * cfg.d_model) * sd["wte.weight"][[ord(c) for c in bias_chars]].sum(0)
    return cfg, sd


def _engine(cfg, sd, dev, kind):
    from lmrl_gym_amd.gpt2 import GPT2Engine
    if kind == "bf16":
        return GPT2Engine(cfg, sd, dev)
    from lmrl_gym_amd.gpt2_f32_engine import GPT2EngineF32
    return GPT2EngineF32(cfg, sd, dev, matmul=kind)


def _random_endgames(pieces, n, seed):
    from lmrl_gym_amd.envs import chess as C
    st = np.random.get_state()
    np.random.seed(seed)
    out = [C.large_piece_random_endgame(pieces) for _ in range(n)]
    np.random.set_state(st)
    return out


def _plan(max_moves):
    """Whole games planned on the host rules: per env (start, [action per turn], [reply index per turn])."""
    import random
    rng = random.Random(7)
    T = max_moves + 1
    plans = []

    def finish(start, acts, reps):
        acts, reps = list(acts), list(reps)
        while len(acts) < T:                      # past the planned moves: junk (never reached when the game ended before)
            acts.append("zz9")
            reps.append(0)
        plans.append((start, acts[:T], reps[:T]))

    mate = next(s for _, s in Board(MATE_IN_ONE).legal() if s.endswith("#"))
    finish(MATE_IN_ONE, [mate], [0])                                                # GAME_OVER, reward +1
    finish(MATE_IN_ONE, ["Qz9", mate], [0, 0])                                      # an illegal string first
    finish(STALEMATING, ["Qb6"], [0])                                               # GAME_OVER by stalemate, reward 0
    b = Board(HANGING)
    assert b.agent("Qa2+")[0] == MOVED
    finish(HANGING, ["Qa2+"], [[u for u, _ in b.legal()].index("b3a2")])            # the reply captures the last piece: bare kings, done
    from lmrl_gym_amd.envs.chess import START_FEN
    b = Board(START_FEN)
    reps = []
    for a, reply in (("f3", "e7e5"), ("g4", "d8h4")):
        assert b.agent(a)[0] == MOVED
        reps.append([u for u, _ in b.legal()].index(reply))
        b.opponent(reply)
    finish(START_FEN, ["f3", "g4"], reps)                                           # fool's mate: the agent is mated, reward -1
    finish(START_FEN, ["e4", "--"], [3, 0])                                         # the null move
    finish(START_FEN, ["Z0"], [0])
    finish(TWO_ROOKS, ["Rd8", "Rad8", "Ke5", "abcdefghijklmnopqrst"], [5, 2, 1, 0])  # ambiguous, legal, illegal, 20-character junk
    finish(START_FEN, ["e5", "Nf3", "Nf3", "O-O", "e4"], [1, 7, 11, 13, 17])        # illegal pawn move, a knight out, then an occupied square, ...
    for k, start in enumerate(_random_endgames("kQK", 6, 11) + _random_endgames("kRK", 5, 12) + [START_FEN] * 3):
        b, acts, reps = Board(start), [], []
        for t in range(T):                        # random legal play with an illegal string now and then (those games reach max_moves)
            lm = b.legal()
            if not lm:
                break
            if rng.random() < 0.25:
                acts.append(rng.choice(["Qh9", "Kk1", "xx", "e9"]))
                reps.append(0)
                continue
            a = rng.choice(lm)[1]
            res, _, d = b.agent(a)
            acts.append(a)
            reps.append(rng.randrange(0, 64))
            if res != MOVED or d:
                break
            lm2 = b.legal()
            _, _, d = b.opponent(lm2[reps[-1] % len(lm2)][0])
            if d:
                break
        finish(start, acts, reps)
    return plans


def test_steered_device_loop_equals_the_env_on_planned_games():
    """The loop steered to planned SAN strings (legal, illegal, ambiguous, junk, null move) with scripted reply indices, then the device's OWN decoded
    action texts fed turn by turn to `VectorChessEnv` with an engine object that returns the same scripted replies: observation, reward, done,
    opponent SAN and episode length equal for every transition; every result code, both signs of the reward and the max_moves ending occur."""
    import torch
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.environment import Text
    from lmrl_gym_amd.envs import chess as C
    dev = _lib.require_gpu()
    max_moves = 5
    plans = _plan(max_moves)
    # ---- the plan itself, on the host rules: it contains what the test is about
    sims = [host_game(s, a, r, max_moves) for s, a, r in plans]
    flat = [x for g in sims for x in g]
    assert {x[2] for x in flat} == {ILLEGAL, MOVED, GAME_OVER, NULL_MOVE}
    assert any(x[3] == 1.0 for x in flat) and any(x[3] == -1.0 and x[2] == MOVED for x in flat)
    assert any(len(g) == max_moves + 1 and not any(x[4] for x in g[:-1]) and g[-1][2] in (ILLEGAL, MOVED) and g[-1][3] != 1.0 for g in sims)
    B, T = len(plans), max_moves + 1
    tok = ByteTokenizer()
    cfg, sd = _weights("tiny", len(tok) + 3, boost=0.0)
    env = C.VectorChessEnv(max_moves=max_moves, random_opponent=True)
    eng = ChessRolloutEngine(_engine(cfg, sd, dev, "bf16"), tok, env, B, max_new_tokens=44, eos_token_id=tok.eos_token_id, max_input_length=256)
    assert eng.T == T
    eng.set_scripted_actions([[plans[b][1][t] for b in range(B)] for t in range(T)], strength=40.0)
    reply_idx = np.array([[plans[b][2][t] for b in range(B)] for t in range(T)], dtype=np.int32)
    eng.set_scripted_replies(reply_idx)
    options = [dict(from_position=p[0]) for p in plans]
    eng.run_episode([0] * B, options, temperature=0.0, use_graph=True, sync_every=0)
    torch.cuda.synchronize()
    recs, inter = eng.records(), eng.interactions()
    # ---- the steering worked: the device played the planned games
    for b, g in enumerate(sims):
        assert recs[b]["action"] == [x[1][:15] for x in g], (b, recs[b]["action"], g)
        assert recs[b]["fen"] == [x[0] for x in g] and recs[b]["final_fen"] == g[-1][6], (b, recs[b]["fen"])
        assert recs[b]["result"].tolist() == [x[2] for x in g] and recs[b]["reward"].tolist() == [x[3] for x in g], b
        assert recs[b]["done"].tolist() == [x[4] for x in g] and recs[b]["opp_san"] == [x[5] or "" for x in g], b
    # ---- the device's own action texts through VectorChessEnv
    pool = ScriptedPool(reply_idx)
    venv = C.VectorChessEnv(max_moves=max_moves, engine=pool)
    hist = venv.reset([None] * B, options)
    done = [False] * B
    n_trans = 0
    for t in range(T):
        if all(done):
            break
        for b in range(B):
            assert (len(inter[b]) > t) == (not done[b]), (b, t)
        acts = [tuple(hist[b]) + (inter[b][t].post_action_history[-1],) if not done[b] else None for b in range(B)]
        pool.turn, pool.asking = t, [b for b in range(B) if not done[b] and recs[b]["result"][t] == MOVED]
        out = venv.step(acts, list(done))
        for b in range(B):
            if done[b]:
                assert out[b] is None
                continue
            tr = inter[b][t]
            assert tr.pre_action_history == tuple(hist[b]) and tr.post_action_history == acts[b], (b, t)
            nh, r, d = out[b]
            assert tr.post_transition_history == tuple(nh) and tr.reward == r and tr.done == d, (b, t, tr, out[b])
            assert (venv.last_opponent_moves[b] or "") == recs[b]["opp_san"][t], (b, t)
            assert isinstance(tr.post_action_history[-1], Text) and tr.post_action_history[-1].is_action
            hist[b], done[b] = nh, d
            n_trans += 1
    assert all(done) and [len(x) for x in inter] == [len(g) for g in sims] and n_trans == len(flat)
    # ---- coverage, from what the device recorded
    results = np.concatenate([r["result"] for r in recs])
    rewards = np.concatenate([r["reward"] for r in recs])
    assert set(results.tolist()) == {ILLEGAL, MOVED, GAME_OVER, NULL_MOVE}
    assert (rewards == 1.0).any() and ((rewards == -1.0) & (results == MOVED)).any()
    assert any(len(r["result"]) == T and not r["done"][:-1].any() and r["result"][-1] in (ILLEGAL, MOVED) and r["done"][-1] for r in recs)
    assert any(o for r in recs for o in r["opp_san"])
    eng.close()


@pytest.mark.parametrize("width,kind,B,max_in,max_new,max_moves,reuse", [("tiny", "bf16", 24, 256, 6, 4, True), ("tiny", "f32", 24, 256, 6, 4, True),
                                                                        ("tiny", "bf16", 24, 40, 6, 3, True), ("tiny", "bf16", 24, 256, 6, 4, False),
                                                                        ("small", "bf16", 256, 256, 4, 2, True), ("small", "f32", 256, 256, 3, 1, True)])
def test_greedy_device_loop_equals_generic_text_path(width, kind, B, max_in, max_new, max_moves, reuse):
    """Same weights, greedy decoding, per-env distinct start FENs of different lengths, the same deterministic reply object on both sides: the
    device loop's transitions == `interact_environment(VectorChessEnv, GPT2PPOPolicy)`, with the policy's default prefill (the K/V rows of the
    longest common prefix of consecutive prompts are kept: `lmrl_chess_tok_prefix` follows the same rule, so both sides forward the same chunks)
    and with `reuse_kv=False` on both sides (every turn from position 0).  max_in = 40: every prompt is left-truncated."""
    import torch
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.envs import chess as C
    from lmrl_gym_amd.policies import GPT2PPOPolicy
    dev = _lib.require_gpu()
    tok = ByteTokenizer()
    cfg, sd = _weights(width, len(tok) + 3, seed=2)
    engine = _engine(cfg, sd, dev, kind)
    starts = ([C.START_FEN, MATE_IN_ONE, TWO_ROOKS, "r3k2r/pppq1ppp/2n2n2/3Pp3/8/2N2N2/PPP2PPP/R3K2R w KQkq e6 0 10"] +
              _random_endgames("kQK", B, 3) + _random_endgames("kRK", B, 4))
    starts = [starts[i % len(starts)] if i < 8 else starts[4 + (i * 7) % (2 * B)] for i in range(B)]
    assert len({len(s) for s in starts}) >= 4
    options = [dict(from_position=s) for s in starts]
    T = max_moves + 1
    REPLY = 5                                      # the deterministic opponent of both sides: legal move number 5 mod count of the position

    class Pool(ScriptedPool):
        def best_moves(self, games):
            out = []
            for start, moves in games:
                b = Board(start)
                for mv in moves:
                    b.opponent(mv)
                lm = b.legal()
                out.append(lm[REPLY % len(lm)][0])
            return out
    env = C.VectorChessEnv(max_moves=max_moves, random_opponent=True)
    eng = ChessRolloutEngine(engine, tok, env, B, max_new_tokens=max_new, eos_token_id=tok.eos_token_id, max_input_length=max_in, reuse_kv=reuse)
    eng.set_scripted_replies(np.full((T, B), REPLY, dtype=np.int32))
    eng.run_episode([0] * B, options, temperature=0.0, use_graph=True, sync_every=0)
    torch.cuda.synchronize()
    mine, recs = eng.interactions(), eng.records()
    pool = Pool(None)
    pol = GPT2PPOPolicy(engine, tok, max_input_length=max_in, max_new_tokens=max_new, do_sample=False, eos_token_id=tok.eos_token_id,
                        out_str_process=lambda x: x.removesuffix("\n") + "\n", reuse_kv=reuse)
    venv = C.VectorChessEnv(max_moves=max_moves, engine=pool)
    ref = E.interact_environment(venv, pol, env_seed=[None] * B, env_options=options, bsize=B)
    assert len(mine) == len(ref) == B
    n_steps = 0
    for b, (x, y) in enumerate(zip(mine, ref)):
        assert len(x) == len(y), (b, len(x), len(y))
        for i, (tx, ty) in enumerate(zip(x, y)):
            assert tx == ty, (b, i, tx, ty)
            n_steps += 1
    texts = {t.post_action_history[-1].text for ep in mine for t in ep}
    keep = eng.traj["keep"].cpu().numpy()
    assert (keep.max() > 0) == reuse                # (the last turn's kept prefix: whole prompts after the illegal strings a random model spells)
    print(f"[chess greedy {width} {kind} B={B} max_in={max_in} reuse={reuse}] kept prefix max={keep.max()} transitions={n_steps} distinct actions={len(texts)} "
          f"results={np.bincount(np.concatenate([r['result'] for r in recs]), minlength=4).tolist()}")
    assert n_steps >= B and len(texts) >= 2
    if max_in == 40:
        assert min(len(tok.encode(C.preprocess_state_og(s))) for s in starts) > max_in
    eng.close()


def _sampled_setup(dev, B=48, max_moves=6, max_new=8, opponent="device"):
    from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.envs import chess as C
    tok = ByteTokenizer()
    cfg, sd = _weights("tiny", len(tok) + 3, seed=5, boost=0.0)
    env = C.VectorChessEnv(max_moves=max_moves, random_opponent=True)
    eng = ChessRolloutEngine(_engine(cfg, sd, dev, "bf16"), tok, env, B, max_new_tokens=max_new, eos_token_id=tok.eos_token_id, max_input_length=256,
                             opponent=opponent)
    starts = (_random_endgames("kQK", B, 21) + _random_endgames("kRK", B, 22))[::2][:B - 4] + [C.START_FEN] * 4
    # mostly legal play, so that the opponent moves: every env is steered to a legal move of its START position in turn 0 and to king / queen / rook
    # steps that are often legal afterwards; whatever the sampler makes of it is what gets replayed below
    import random
    rng = random.Random(9)
    script = []
    for t in range(eng.T):
        row = []
        for s in starts:
            lm = Board(s).legal()
            row.append(rng.choice(lm)[1] if t == 0 else rng.choice([m for _, m in lm] + ["Kd4", "Ke5", "Qd4", "Rd4", "Nf3", "e4", "d4"]))
        script.append(row)
    eng.set_scripted_actions(script, strength=12.0)
    return eng, tok, cfg, sd, starts


def _snapshot(eng):
    import torch
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy().copy() for k, v in eng.traj.items()}
    nt = h["n_turns"]
    live = np.arange(eng.T)[None, :] < nt[:, None]
    out = dict(n_turns=nt, ep_reward=h["ep_reward"], cur_fen=h["cur_fen"])
    for k in ("gen_len", "result", "reward", "done"):
        out[k] = np.where(live, h[k], 0)
    for k in ("fen", "action", "opp_san", "reply"):
        out[k] = np.where(live[:, :, None], h[k], 0)
    tokm = live[:, :, None] & (np.arange(eng.max_new)[None, None, :] < h["gen_len"][:, :, None])
    out["gen"] = np.where(tokm, h["gen"], 0)
    return out


def test_graph_replay_equals_eager_and_the_device_opponent_draws_the_documented_stream():
    """Sampled episodes with the device opponent: graph replay == eager launches bit for bit; a second replay under a new episode number draws other
    replies; every reply is `legal_moves[(word * count) >> 32]` of its position for the Philox word documented in include/lmrl_amd.h (restated on
    the host: oracle/gpt2.py), found by replaying the record on the host rules."""
    from lmrl_gym_amd import _lib
    sys.path.insert(0, ROOT)
    from oracle.gpt2 import philox4x32_10
    dev = _lib.require_gpu()
    eng, tok, cfg, sd, starts = _sampled_setup(dev)
    B = eng.B
    options = [dict(from_position=s) for s in starts]
    seed, episode = (7 << 32) | 12345, 3
    eng.run_episode([0] * B, options, temperature=1.0, sample_seed=seed, episode=episode, use_graph=False, sync_every=0)
    eager = _snapshot(eng)
    eng.run_episode([0] * B, options, temperature=1.0, sample_seed=seed, episode=episode, use_graph=True, sync_every=0)
    graph = _snapshot(eng)
    for k in eager:
        assert np.array_equal(eager[k], graph[k]), k
    recs = eng.records()
    eng.run_episode([0] * B, options, temperature=1.0, sample_seed=seed, episode=episode + 1, use_graph=True, sync_every=0)
    other = _snapshot(eng)
    assert not np.array_equal(other["reply"], graph["reply"])
    # ---- the reply stream, replayed on the host rules
    n_replies = 0
    for b, r in enumerate(recs):
        board = Board(starts[b])
        for t in range(len(r["result"])):
            assert board.fen() == r["fen"][t] or t == 0, (b, t)
            res, _, _ = board.agent(r["action"][t])
            assert res == r["result"][t], (b, t)
            if res != MOVED:
                assert r["reply"][t] == "" and r["opp_san"][t] == ""
                continue
            lm = board.legal()
            word = int(philox4x32_10(b, t, 0x43484553, (episode << 12) + t, seed & 0xFFFFFFFF, seed >> 32, rounds=7)[0])
            want = lm[(word * len(lm)) >> 32]
            assert (r["reply"][t], r["opp_san"][t]) == want, (b, t, r["reply"][t], want)
            san, rew, _ = board.opponent(want[0])
            assert san == r["opp_san"][t] and rew == r["reward"][t]
            n_replies += 1
    print(f"[chess reply stream] replies checked: {n_replies}")
    assert n_replies >= B
    eng.close()


def test_host_engine_pool_turns_equal_the_device_opponent_on_the_same_replies():
    """The two-launch turn around the host hand-off (an `EnginePool`-like object: moves [B][8] down, replies [B][8] up) records what the one-launch
    turn with the device opponent records when both answer with the same move (legal move number 5 mod count); an illegal reply raises."""
    from lmrl_gym_amd import _lib
    dev = _lib.require_gpu()

    class Pool:
        calls, bad = 0, False

        def best_moves(self, games):
            self.calls += 1
            out = []
            for start, moves in games:
                b = Board(start)
                for mv in moves:
                    b.opponent(mv)
                lm = b.legal()
                out.append("a1a1" if self.bad else lm[5 % len(lm)][0])
            return out
    pool = Pool()
    snaps = []
    for opp in ("device", pool):
        eng, tok, cfg, sd, starts = _sampled_setup(dev, B=24, max_moves=4, opponent=opp)
        options = [dict(from_position=s) for s in starts]
        if opp == "device":
            eng.set_scripted_replies(np.full((1, eng.B), 5, dtype=np.int32))
        eng.run_episode([0] * eng.B, options, temperature=1.0, sample_seed=11, episode=2, use_graph=False, sync_every=0)
        snaps.append(_snapshot(eng))
        if opp != "device":
            with pytest.raises(_lib.LmrlError):
                eng.run_episode([0] * eng.B, options, use_graph=True)
            pool.bad = True
            with pytest.raises(RuntimeError, match="not legal"):
                eng.run_episode([0] * eng.B, options, temperature=1.0, sample_seed=11, episode=2, use_graph=False, sync_every=0)
        eng.close()
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k], snaps[1][k]), k
    assert pool.calls >= 2 and (snaps[0]["result"] == MOVED).sum() >= eng.B


def test_chess_ppo_records_and_device_ppo_data_equal_the_host_chain_path():
    """`ChessRolloutEngine.ppo_records` == `text_trajectory_chains_from_transitions(interactions)` tokenised (tokens, action flags, reward placement,
    done); the device PPO data built from them == the host-array form on those chains, at the tolerances of the Maze twin of this test; a
    `max_length` that cuts action tokens raises the reference's truncation assert; `text_env_eval` / `ppo_rollouts` summaries."""
    import torch
    from lmrl_gym_amd import _lib, environment as E
    from lmrl_gym_amd.algorithms import ppo
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.algorithms.ppo_inference import GPT2PPOInference, text_trajectory_chains_from_transitions
    from lmrl_gym_amd.chess_rollout import chess_summary
    from lmrl_gym_amd.train.gpt2_f32 import GPT2F32, LinearHeadF32
    dev = _lib.require_gpu()
    eng, tok, cfg, sd, starts = _sampled_setup(dev, B=40, max_moves=5, max_new=6)
    B = eng.B
    options = [dict(from_position=s) for s in starts]
    eng.run_episode([0] * B, options, temperature=1.0, sample_seed=8, use_graph=False, sync_every=0)
    torch.cuda.synchronize()
    inter = eng.interactions()
    chains = [E.TokenTrajectoryChain.from_text_trajectory_chain(c, tok) for c in text_trajectory_chains_from_transitions(inter)]
    rec = eng.ppo_records()
    flat = [tt for c in chains for tt in c.to_list()]
    assert rec.n == len(flat) >= 2 * B and rec.n_chains == B == len(chains)
    h = {k: getattr(rec, k).cpu().numpy() for k in ("tokens", "is_action", "reward", "n_tok", "done", "chain", "pos", "last")}
    k = 0
    n_act_lens = set()
    for c, ch in enumerate(chains):
        lst, p = ch.to_list(), 0
        for i, tt in enumerate(lst):
            n = int(h["n_tok"][k])
            assert n == len(tt.tokens) and h["tokens"][k, :n].tolist() == tt.tokens.tolist(), (c, i)
            assert h["is_action"][k, :n].astype(bool).tolist() == tt.is_action.tolist() and np.array_equal(h["reward"][k, :n], tt.reward)
            assert h["chain"][k] == c and h["pos"][k] == p and bool(h["last"][k]) == (i == len(lst) - 1)
            n_act_lens.add(int(tt.is_action.sum()))
            p += n - 1
            k += 1
        assert bool(h["done"][c]) == bool(lst[-1].done)
    assert len(n_act_lens) >= 2
    g = torch.Generator().manual_seed(6)
    sd2 = {kk: v + 0.02 * torch.randn(v.shape, generator=g) * v.abs().mean().clamp_min(1e-3) for kk, v in sd.items()}
    pol, init = GPT2F32(sd2, cfg.n_head, device=dev), GPT2F32(sd, cfg.n_head, device=dev)
    vh = LinearHeadF32(dict(kernel=torch.randn(cfg.d_model, 1, generator=g) * 0.05, bias=torch.tensor([0.2])), dev)
    inf = GPT2PPOInference(pol, vh, tok.pad_token_id, initial_policy=init)
    kw = dict(gamma=0.97, lam=0.9, kl_weight=0.05)
    max_length = int(h["n_tok"].max()) + 1
    ds, kls = eng.ppo_data(inf, max_length=max_length, bsize=64, **kw)
    datas, kls_h = inf.get_ppo_data_from_token_trajectory_chain(chains, bsize=32, max_length=max_length, **kw)
    host = ppo.PPODataset.from_ppo_data_list(datas, tok, BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, max_length))
    got = ds.to_host()
    assert (got.input_ids == host.input_ids).all() and (got.should_take_action == host.should_take_action).all()
    np.testing.assert_allclose(got.old_logprobs, host.old_logprobs, rtol=0, atol=1e-5)
    np.testing.assert_allclose(got.old_values, host.old_values, rtol=0, atol=1e-5)
    np.testing.assert_allclose(got.old_returns, host.old_returns, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got.old_advantages, host.old_advantages, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(kls.cpu().numpy(), kls_h, rtol=1e-5, atol=5e-6)
    with pytest.raises(ValueError, match="trajectory truncation error"):
        eng.ppo_data(inf, max_length=int(h["n_tok"].min()) - 1, bsize=64, **kw)
    # ---- text_env_eval: a full batch + a partial one, exactly n_rollouts episodes, the chess summary's formulas on the returned interactions
    n_rollouts = B + 9
    eng.set_scripted_actions(None)
    inter2, summ = eng.text_env_eval(n_rollouts, seed_generator=iter(range(1000)), env_options=dict(from_position=MATE_IN_ONE), temperature=1.0, sample_seed=4)
    assert len(inter2) == n_rollouts and all(len(ep) >= 1 for ep in inter2)
    want = chess_summary(inter2)
    rewards = [[t.reward for t in ep] for ep in inter2]
    assert want["victories"]["mean"] == np.mean([1 if 1 in r else 0 for r in rewards])
    assert want["percent_illegals"]["mean"] == np.mean([sum(1 for i, x in enumerate(r) if x == -1 and i < len(r) - 1) / len(r) * 100 for r in rewards])
    assert want["episode_length"]["mean"] == np.mean([len(r) for r in rewards])
    for key in ("reward", "done", "victories", "percent_illegals", "episode_length"):
        assert summ[key] == want[key], key
    assert summ["reward"]["mean"] == np.mean(np.asarray([sum(r) for r in rewards], dtype=np.float32))
    assert summ["done"]["mean"] == np.mean([float(ep[-1].done) for ep in inter2])
    assert all(ep[0].pre_action_history[0].text == " ".join(MATE_IN_ONE) for ep in inter2)
    # ---- one data-collection round of the resident loop
    ds2, kls2, summ2 = eng.ppo_rollouts(inf, n_rollouts, iter(range(1000)), None, max_length=max_length, bsize=64, temperature=1.0, sample_seed=8, **kw)
    sta = ds2.should_take_action
    assert ds2.input_ids.shape[1] == max_length and kls2.numel() == int(sta.sum().item())
    assert abs(ds2.input_ids.shape[0] - n_rollouts * float(summ2["episode_length"]["mean"])) < 1e-3
    adv = ds2.old_advantages[sta.bool()].double()
    assert abs(float(adv.mean())) < 1e-4 and abs(float(adv.var(unbiased=False)) - 1.0) < 1e-3
    eng.close()


def test_engine_refuses_what_is_out_of_scope():
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.chess_rollout import ChessRolloutEngine
    from lmrl_gym_amd.datasets import ByteTokenizer
    from lmrl_gym_amd.environment import Text
    from lmrl_gym_amd.envs import chess as C
    dev = _lib.require_gpu()
    tok = ByteTokenizer()
    cfg, sd = _weights("tiny", len(tok) + 3)
    engine = _engine(cfg, sd, dev, "bf16")
    with pytest.raises(ValueError, match="generic|text_env_eval"):
        ChessRolloutEngine(engine, tok, C.VectorChessEnv(random_opponent=True, state_fn=C.preprocess_state), 4)
    with pytest.raises(ValueError, match="generic|text_env_eval"):
        ChessRolloutEngine(engine, tok, C.VectorChessEnv(random_opponent=True, initial_history=(Text("x", False),)), 4)
    eng = ChessRolloutEngine(engine, tok, C.VectorChessEnv(max_moves=2, random_opponent=True), 4, max_new_tokens=2)
    with pytest.raises(ValueError, match="invalid FEN"):
        eng.run_episode([0] * 4, dict(from_position="not a fen"), max_turns=1)
    eng.close()


def _harness():
    import importlib.util
    spec = importlib.util.spec_from_file_location("harness", os.path.join(ROOT, "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    return H


def test_harness_ppo_chess_device_rollouts(capsys):
    """`scripts/harness.py ppo --env chess --device-rollouts 1` at toy scale: device rollouts feeding the host-array data path, the resident
    iteration over two rounds with the device opponent, and the host engine pool where the reference-built engine binary exists."""
    H = _harness()
    base = ["ppo", "--env", "chess", "--model", "random:tiny", "--n-rollouts", "6", "--rollout-bsize", "4", "--train-bsize", "4", "--ppo-data-bsize", "4",
            "--max-input-length", "192", "--max-output-length", "4", "--chess-pieces", "kQK", "--chess-max-moves", "3", "--device-rollouts", "1"]
    H.main(base + ["--chess-random-opponent", "1", "--resident", "0", "--max-steps", "2"])
    H.main(base + ["--chess-random-opponent", "1", "--resident", "1", "--n-rounds", "2"])
    out = capsys.readouterr().out
    assert out.count('"data_collection"') == 3 and '"device_resident": true' in out and '"eval"' in out


def test_harness_ppo_chess_device_rollouts_with_engine_pool(capsys):
    sf = os.path.join(ROOT, "oracle", "_ref", "stockfish")
    if not os.path.exists(sf):
        pytest.skip("oracle/_ref/stockfish is not built")
    H = _harness()
    H.main(["ppo", "--env", "chess", "--model", "random:tiny", "--n-rollouts", "4", "--rollout-bsize", "4", "--train-bsize", "4", "--ppo-data-bsize", "4",
            "--max-input-length", "192", "--max-output-length", "4", "--chess-pieces", "kQK", "--chess-max-moves", "2", "--device-rollouts", "1",
            "--chess-engine", sf, "--chess-use-nnue", "false", "--chess-movetime-ms", "5", "--resident", "1", "--max-steps", "1"])
    assert '"device_resident": true' in capsys.readouterr().out
