"""Beam-search oracle (TEST INFRASTRUCTURE): the rules of HF-Flax `_beam_search` as transformers 4.26.1 runs it, restated in plain numpy with float64
arithmetic (DESIGN.md "Beam search"; restated from the published source, unverified against the library, which is not installed).

Everything is literal: the -1e7 penalties are ADDED (float64 keeps the sums apart), every top-k is a stable sort (ties to the lower index), and the
loop condition is global over the batch.  `logits_fn(seqs)` gets the generated tokens of the B * K running beams (row = item * K + beam) and
returns their next-token logits [B * K, V]."""
import numpy as np

from lmrl_gym_amd.beam import BEST_RUNNING_BEAM       # index of the running beam the loop condition reads: one constant with the kernel side

NEG = -1.0e7


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _top(values, k):
    """Indices of the k largest entries in descending order, ties to the lower index."""
    return np.argsort(-np.asarray(values, dtype=np.float64), kind="stable")[:k]


class State:
    def __init__(self, B, K):
        self.B, self.K = B, K
        self.run_seq = [[[] for _ in range(K)] for _ in range(B)]
        self.run_score = np.tile(np.array([0.0] + [NEG] * (K - 1)), (B, 1))
        self.fin_seq = [[[] for _ in range(K)] for _ in range(B)]
        self.fin_score = np.full((B, K), NEG)
        self.fin_flag = np.zeros((B, K), dtype=bool)

    def copy(self):
        s = State(self.B, self.K)
        s.run_seq = [[list(x) for x in r] for r in self.run_seq]
        s.fin_seq = [[list(x) for x in r] for r in self.fin_seq]
        s.run_score, s.fin_score, s.fin_flag = self.run_score.copy(), self.fin_score.copy(), self.fin_flag.copy()
        return s


def keep_going(st, t, max_new_tokens, P, length_penalty, early_stopping):
    """The loop condition, evaluated before generated position t."""
    if not t < max_new_tokens:
        return False
    if st.fin_flag.all() and early_stopping:
        return False
    best_running = st.run_score[:, BEST_RUNNING_BEAM] / float(P + max_new_tokens) ** length_penalty                  # [B]
    worst_finished = np.where(st.fin_flag, st.fin_score.min(axis=1, keepdims=True), NEG)                             # [B, K]
    return bool((worst_finished < best_running[:, None]).any())


def step(st, logits, t, P, eos, length_penalty, early_stopping, logprobs=False):
    """One body at position t on logits [B * K, V] (logprobs=True: they already are log-probabilities and are taken as they stand).  Returns (new state, info) with info[b] = dict(cand_score, cand_beam, cand_tok, parent, tok,
    gap): `parent` / `tok` of the next running beams (parent as a beam index of the item) and `gap`, the smallest difference between adjacent
    candidates among the item's top 2K + 1."""
    B, K = st.B, st.K
    lp_all = (np.asarray(logits, dtype=np.float64) if logprobs else log_softmax(logits)).reshape(B, K, -1)
    V = lp_all.shape[-1]
    new, info = st.copy(), []
    for b in range(B):
        flat = (lp_all[b] + st.run_score[b][:, None]).reshape(-1)
        order = _top(flat, min(2 * K + 1, flat.size))
        top = order[: 2 * K]
        gaps = -np.diff(flat[order])
        cand_score, cand_beam, cand_tok = flat[top], top // V, top % V
        just_finished = cand_tok == eos
        pick = _top(cand_score + just_finished * NEG, K)
        new.run_score[b] = (cand_score + just_finished * NEG)[pick]
        new.run_seq[b] = [st.run_seq[b][cand_beam[j]] + [int(cand_tok[j])] for j in pick]
        norm = cand_score / float(P + t) ** length_penalty
        full = bool(st.fin_flag[b].all()) and early_stopping
        norm = norm + (~just_finished | full) * NEG
        m_score = np.concatenate([st.fin_score[b], norm])
        m_flag = np.concatenate([st.fin_flag[b], just_finished])
        m_seq = st.fin_seq[b] + [st.run_seq[b][cand_beam[j]] + [int(cand_tok[j])] for j in range(len(top))]
        keep = _top(m_score, K)
        new.fin_score[b], new.fin_flag[b], new.fin_seq[b] = m_score[keep], m_flag[keep], [list(m_seq[j]) for j in keep]
        info.append(dict(cand_score=cand_score, cand_beam=cand_beam, cand_tok=cand_tok, parent=cand_beam[pick], tok=cand_tok[pick],
                         gap=float(gaps.min()) if gaps.size else np.inf))
    return new, info


def result(st, eos):
    """Per item (sequence cut behind the first eos, score)."""
    out = []
    for b in range(st.B):
        seq, score = (st.fin_seq[b][0], st.fin_score[b][0]) if st.fin_flag[b].any() else (st.run_seq[b][0], st.run_score[b][0])
        seq = list(seq)
        if eos in seq:
            seq = seq[: seq.index(eos) + 1]
        out.append((seq, float(score)))
    return out


def beam_search(logits_fn, B, K, P, max_new_tokens, eos, length_penalty=1.0, early_stopping=False, on_step=None, stop_rule=True):
    """Returns (sequences, scores, steps run, smallest candidate gap per item).  on_step(t, state before, info, state after) is called per position.
    Position 0 always runs: the library runs the first body outside its while loop for prompts longer than one token (before it, the last running
    beam and every pool entry stand at -1e7, and with length_penalty = 0 the strict comparison of the loop condition would not even start).
    stop_rule=False: all max_new_tokens positions run (the body's rules alone)."""
    st, t, gaps = State(B, K), 0, np.full(B, np.inf)
    while t < max_new_tokens and (t == 0 or not stop_rule or keep_going(st, t, max_new_tokens, P, length_penalty, early_stopping)):
        logits = np.asarray(logits_fn([s for b in range(B) for s in st.run_seq[b]]), dtype=np.float64)
        new, info = step(st, logits, t, P, eos, length_penalty, early_stopping)
        gaps = np.minimum(gaps, [i["gap"] for i in info])
        if on_step is not None:
            on_step(t, st, info, new)
        st, t = new, t + 1
    res = result(st, eos)
    return [r[0] for r in res], np.array([r[1] for r in res]), t, gaps
