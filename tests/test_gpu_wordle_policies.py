"""GPU tier: the scripted Wordle policies' kernels and the device-resident episode loop (csrc/wordle_policy.hip) against the
reference-generated fixtures (tests/golden/wordle_scripted_policies.json) and the host faces of the same core."""
import ctypes
import json

import numpy as np
import pytest

import lmrl_gym_amd  # noqa: F401
from test_wordle_policies import G, _mt, _ptr, build_policy, case_vocab

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _episodes(rec):
    return [rec.episode(i) for i in range(len(rec))]


@pytest.mark.parametrize("case", G["cases"], ids=[c["name"] for c in G["cases"]])
def test_device_episode_loop_equals_the_reference_episodes(case):
    """All fixture episodes of the case in ONE batch: action for action, observation, reward and done — eagerly and as a replayed graph."""
    from lmrl_gym_amd.envs import wordle_policies as P
    vocab = case_vocab(case)
    eps = case["episodes"]
    loop = P.WordleScriptedRollouts(vocab, build_policy(case["policy"], vocab), len(eps))
    seeds = [ep["env_seed"] for ep in eps], [ep["policy_seed"] for ep in eps]
    for use_graph in (False, True):
        got = _episodes(loop.run(*seeds, use_graph=use_graph))
        assert len(got) == len(eps)
        for (actions, obs, rewards, done), ep in zip(got, eps):
            assert actions == ep["actions"] and obs == ep["observations"] and rewards == ep["rewards"] and done == ep["done"]
    loop.close()


def _act_vs_host(vocab, policy, guesses_before, n, seed0):
    """n envs stepped through `guesses_before`, then one act on the device and one on the host faces from the same state and streams."""
    from lmrl_gym_amd import _lib
    from lmrl_gym_amd.envs import wordle as W, wordle_policies as P
    L = _lib.lib()
    dev = _lib.require_gpu()
    words, V = P.packed_vocab(vocab), len(vocab.all_vocab)
    logtab = P.log_table(V)
    env = W.VectorWordleEnv(vocab, reformat=False)
    env.reset_device(np.arange(seed0, seed0 + n, dtype=np.uint64))
    for g in guesses_before:
        env.step_device(torch.full((n,), W.pack_guess(g), dtype=torch.int32, device=dev))
    pol_seeds = np.arange(7000 + seed0, 7000 + seed0 + n, dtype=np.uint64)
    mt_pol = torch.zeros(L.lmrl_mt_bytes(n), dtype=torch.uint8, device=dev)
    _lib.check(L.lmrl_mt_seed(_lib.ptr(mt_pol), _lib.ptr(torch.from_numpy(pol_seeds.view(np.int64)).to(dev)), None, n, _lib.stream_ptr()))
    scratch = torch.zeros(L.lmrl_wordle_policy_scratch_bytes(n, V), dtype=torch.uint8, device=dev)
    logtab_d = torch.from_numpy(logtab).to(dev)
    guess = torch.full((n,), -1, dtype=torch.int32, device=dev)
    df, dn = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    di = torch.zeros(n, dtype=torch.float64, device=dev)
    desc = policy.descriptor()
    state = env.state.view(torch.int32).view(19, n).cpu().numpy().view(np.uint32)
    _lib.check(L.lmrl_wordle_policy_act(env._ctx, ctypes.byref(desc), _lib.ptr(env.state), _lib.ptr(env.mt), _lib.ptr(mt_pol), None, _lib.ptr(logtab_d),
                                        _lib.ptr(scratch), scratch.numel(), _lib.ptr(guess), _lib.ptr(df), _lib.ptr(dn), _lib.ptr(di), n,
                                        _lib.stream_ptr()), "lmrl_wordle_policy_act")
    guess, df, dn, di = guess.cpu().numpy().view(np.uint32), df.cpu().numpy(), dn.cpu().numpy(), di.cpu().numpy()
    n_ties = 0
    for e in range(n):
        masks = np.ascontiguousarray(state[:10, e])
        f, nb, info = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        g = L.lmrl_wordle_policy_host_act(ctypes.byref(desc), _ptr(words), V, _ptr(masks), int(state[11, e]), _ptr(logtab), _ptr(_mt(0)),
                                          _ptr(_mt(int(pol_seeds[e]))), ctypes.byref(f), ctypes.byref(nb), None, ctypes.byref(info))
        assert (int(guess[e]), int(df[e]), int(dn[e])) == (g, f.value, nb.value), e
        assert float.hex(float(di[e])) == float.hex(info.value), e
        n_ties += nb.value > 1
    env.close()
    return n_ties


def test_act_kernel_equals_host_face():
    from lmrl_gym_amd.envs import wordle as W, wordle_policies as P
    big = W.Vocabulary.builtin("wordle_official.txt")
    assert big.all_vocab_size() == 2315
    ties = _act_vs_host(big, P.OptimalPolicy(big, P.StartWordPolicy(["raise"])), ["raise"], 256, 100)
    assert ties > 0
    small = W.Vocabulary.builtin("wordle_official_400.txt")
    _act_vs_host(small, P.OptimalPolicy(small), [], 4, 300)       # the full first-turn sweep


@pytest.mark.parametrize("name", ["mixture_p0.5", "optimal_default_start_64", "coin_optimal_mixture_64"])
def test_policies_under_interact_environment_give_the_loops_episodes(name):
    from lmrl_gym_amd import environment as E
    from lmrl_gym_amd.envs import wordle as W
    case = next(c for c in G["cases"] if c["name"] == name)
    vocab = case_vocab(case)
    eps = case["episodes"][:16]
    env = W.VectorWordleEnv(vocab, reformat=False)
    policy = build_policy(case["policy"], vocab).attach(env).seed([ep["policy_seed"] for ep in eps])
    inter = E.interact_environment(env, policy, env_seed=[ep["env_seed"] for ep in eps], bsize=len(eps))
    for trs, ep in zip(inter, eps):
        assert [t.post_action_history[-1].text for t in trs] == ep["actions"]
        assert [t.post_transition_history[-1].text for t in trs] == ep["observations"]
        assert [float(t.reward) for t in trs] == ep["rewards"] and trs[-1].done == ep["done"]
    env.close()


def test_device_dataset_replays_on_the_oracle_env_and_feeds_ilql(tmp_path):
    """OptimalPolicy draws on the policy stream only, so its episodes replay on the oracle env from the env seeds alone; the default
    start words bring the invalid-word branch in (25 of the 28 are not in the 431-word list)."""
    from lmrl_gym_amd import datasets as DS
    from lmrl_gym_amd.algorithms.common import BlockingStrategy, Padding, Truncation
    from lmrl_gym_amd.envs import wordle as W, wordle_policies as P
    from oracle.wordle import OracleWordleEnv
    vocab = W.Vocabulary.builtin("wordle_official_400.txt")
    policy = P.OptimalPolicy(vocab, P.StartWordPolicy())
    items, seeds, _ = DS.generate_wordle_dataset_device(vocab, 150, policy, seed=4, bsize=64, return_seeds=True)
    assert len(items) == 150 and len(seeds) == 150
    import random
    r = random.Random(4)
    assert seeds == [r.randint(0, 2 ** 31 - 1) for _ in range(150)]          # PolicyDataGenerator's env-seed sequence (data.py:27)
    wins = invalid = 0
    for it, sd in zip(items, seeds):
        o = OracleWordleEnv(vocab.all_vocab, True, -1.0)
        hist = o.reset(sd)
        seq, rew = it["sequence"], it["reward"]
        assert seq[0] == ("Wordle:\n", 0.0) and len(rew) == len(seq) - 1 and it["done"]
        done, k = False, 1
        while not done:
            hist, r_, done = o.step(hist + ((seq[k][0], True),))
            assert seq[k][1] == 1.0 and seq[k + 1] == (hist[-1][0], 0.0)
            assert rew[k - 1] == float(r_) and rew[k] == 0.0
            invalid += seq[k + 1][0] == "\n"
            k += 2
        assert k == len(seq)
        wins += rew[-2] == 0.0
    assert wins >= 140 and invalid > 0
    p = tmp_path / "optimal.jsonl"
    DS.write_jsonl(str(p), items)
    ds = DS.ilql_dataset_from_jsonl(str(p), DS.WordleTokenizer(), BlockingStrategy(Padding.RIGHT, Truncation.RIGHT, 80))
    assert len(ds) == 150
    mix = DS.generate_wordle_dataset_device(vocab, 70, P.RandomMixturePolicy(0.5, vocab), seed=1, bsize=32)
    assert len(mix) == 70 and all(it["done"] and len(it["reward"]) == len(it["sequence"]) - 1 for it in mix)


def test_harness_gen_data_and_optimal_perf(tmp_path, capsys):
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("harness", os.path.join(os.path.dirname(__file__), "..", "scripts", "harness.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    out = tmp_path / "d.jsonl"
    for pol in ("mixture", "optimal", "optimal-mixture"):
        H.main(["gen-data", "--n-data", "40", "--policy", pol, "--start-word", "raise", "--device-loop", "1", "--bsize", "32", "--out", str(out)])
        assert sum(1 for _ in open(out)) == 40
    H.main(["optimal-perf", "--n", "200", "--bsize", "128"])
    logs = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    perf = next(l["optimal_perf"] for l in logs if "optimal_perf" in l)
    assert perf["n"] == 200 and perf["solved"] > 0.95 and -5.0 < perf["reward_mean"] < -1.0
