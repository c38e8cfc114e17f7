"""Rollout records -> the blocked ILQL / MC / BC datasets without leaving the device (csrc/offline_data.hip).

The offline trainers of the reference read jsonl text (`wordle/misc/data_gen.py:53-62`), re-tokenise every episode and block
`ILQLData.from_token_trajectory_chain` / `MCData.from_token_trajectory_chain` (ilql/data.py:18-79, mc_returns/data.py:21-74) or the
(ids, training mask) pairs of the BC scripts with numpy.  The device loops of this package already leave `TokenTrajectory` fields in HBM
(`PPORecords`: `WordleScriptedRollouts.token_records()`, `WordleRolloutEngine.ppo_records()`, the Maze and chess engines' records), so here

    records --lmrl_offline_block--> input_ids, should_take_action, rewards, dones (+ next_token_ids / next_dones on chains)   DeviceILQLDataset
    records --lmrl_rtg, lmrl_offline_block--> input_ids, should_take_action, returns                                          DeviceMCDataset
    records --lmrl_offline_block--> input_ids, input_training_mask                                                            DeviceMaskDataset
    records --lmrl_record_returns--> one score per chain --host decision on [n_chains] floats--> kept rows                    filter_records

mirror `ppo_device.DevicePPODataset`: `FIELDS`, `concat`, `trimmed_width`, `batch`, `batches`, `to_host` (the existing `ILQLDataset` /
blocked-MC dict / `MaskDataset`, for parity tests and pickling).  Only `Padding.RIGHT` with `Truncation.RIGHT` or `Truncation.LEFT` is built
(the strategies the task scripts use); anything else raises.  `GPT2ILQLTrain.step`, `GPT2MCTrain.step` and `GPT2BCTrain.step` take a
device batch as they take a numpy batch (`step(**ds.batch(index))`), with the same loss, logs, gradients and update, bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np

from .. import _lib
from .common import BlockingStrategy, Padding, Truncation
from .ppo_device import PPORecords


class _CBlocks(ctypes.Structure):             # lmrl_offline_blocks (include/lmrl_amd.h)
    _fields_ = [(n, ctypes.c_void_p) for n in ("input_ids", "should_take_action", "rewards", "returns", "training_mask", "dones", "lengths",
                                                "next_token_ids", "next_dones", "next_lengths")]


def _strategy(blocking_strategy: BlockingStrategy, rec: PPORecords):
    """-> (width T, truncate_left).  max_length None: the longest trajectory of the records (one 4-byte readback)."""
    if blocking_strategy.padding != Padding.RIGHT:
        raise ValueError("the device data build pads on the right (Padding.RIGHT); Padding.LEFT is only built on the host")
    if blocking_strategy.truncation not in (Truncation.RIGHT, Truncation.LEFT):
        raise ValueError(f"unknown truncation {blocking_strategy.truncation!r}")
    T = blocking_strategy.max_length
    if T is None:
        T = max(int(rec.n_tok.max().item()), 2)
    if int(T) < 2:
        raise ValueError("max_length must be at least 2 (the shifted arrays have max_length - 1 columns)")
    return int(T), blocking_strategy.truncation == Truncation.LEFT


class ValidatedKeep:
    """What `filter_records` returns: the kept rows (int32 device tensor `rows`, host copy `rows_host`) of the records they were chosen from.
    The builders take it as `keep=` without checking it again."""

    def __init__(self, rows, rows_host: np.ndarray, rec: PPORecords):
        self.rows, self.rows_host, self.rec = rows, rows_host, rec

    def __len__(self):
        return int(self.rows_host.size)


def _keep_tensor(keep, rec: PPORecords):
    """The kept-row list as an int32 device tensor, refused when an index lies outside the records or when it takes some but not all
    trajectories of a chain (the next-token rule and a chain's `done` need whole chains).  The check reads [n] integers, no token data."""
    import torch
    if keep is None:
        return None
    if isinstance(keep, ValidatedKeep):          # `filter_records` made it from these records: nothing to read back
        if keep.rec is not rec:
            raise ValueError("this keep list was made by filter_records for other records")
        return keep.rows
    if not isinstance(keep, torch.Tensor):
        keep = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.int32)).to(rec.tokens.device)
    keep = keep.to(torch.int32).contiguous()
    if keep.numel() == 0:
        raise ValueError("no row is kept: nothing to build a dataset from")
    kh = keep.cpu().numpy()
    if int(kh.min()) < 0 or int(kh.max()) >= rec.n:
        raise ValueError(f"keep holds row indices outside the records (0 .. {rec.n - 1})")
    if rec.chain is not None:
        ch = rec.chain.cpu().numpy()
        kept, total = np.bincount(ch[kh], minlength=rec.n_chains), np.bincount(ch, minlength=rec.n_chains)
        if ((kept != 0) & (kept != total)).any():
            raise ValueError("keep splits a chain: keep every trajectory of a chain or none (`filter_records` does)")
    return keep


def block_records(rec: PPORecords, T: int, pad: int, truncate_left: bool, fields: Sequence[str], keep=None, returns=None) -> Dict[str, "torch.Tensor"]:
    """`lmrl_offline_block`: the named outputs (+ `lengths`, and `next_lengths` with `next_token_ids`) for the kept rows, as device tensors."""
    import torch
    dev = rec.tokens.device
    keep = _keep_tensor(keep, rec)
    if keep is not None and keep.numel() == 0:
        raise ValueError("no row is kept: nothing to build a dataset from")
    m = rec.n if keep is None else int(keep.numel())
    shapes = dict(input_ids=((m, T), torch.int32), should_take_action=((m, T - 1), torch.uint8), rewards=((m, T - 1), torch.float32),
                  returns=((m, T - 1), torch.float32), training_mask=((m, T), torch.float32), dones=((m,), torch.uint8), lengths=((m,), torch.int32),
                  next_token_ids=((m, T), torch.int32), next_dones=((m,), torch.uint8), next_lengths=((m,), torch.int32))
    want = set(fields) | {"input_ids", "lengths"}
    if "next_token_ids" in want:
        want |= {"next_dones", "next_lengths"}
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in shapes if k in want}
    cb = _CBlocks(**{k: _lib.ptr(v) for k, v in out.items()})
    c = rec.c_struct()
    pitch = 0 if returns is None else int(returns.shape[1])
    assert returns is None or (returns.is_contiguous() and int(returns.shape[0]) == rec.n)
    _lib.check(_lib.lib().lmrl_offline_block(ctypes.byref(c), _lib.ptr(keep), 0 if keep is None else m, int(T), int(pad), int(bool(truncate_left)),
                                             _lib.ptr(returns), pitch, ctypes.byref(cb), _lib.stream_ptr()), "lmrl_offline_block")
    return out


class _DeviceDataset:
    """Blocked arrays in HBM: `FIELDS` (the first is input_ids [N, T]); fields named in `WIDE` have T columns, `ROW` fields one value per row,
    every other field T - 1 columns.  `lengths` int32 [N] = every row's token count as the build saw it."""
    FIELDS: tuple = ()
    WIDE: tuple = ("input_ids",)
    ROW: tuple = ()

    def __init__(self, longest: Optional[int] = None, lengths=None, **arrays):
        self.fields = tuple(k for k in self.FIELDS if arrays.get(k) is not None)
        for k in self.FIELDS:
            setattr(self, k, arrays.get(k))
        n, t = self.input_ids.shape
        for k in self.fields:
            want = (n,) if k in self.ROW else ((n, t) if k in self.WIDE else (n, t - 1))
            assert tuple(getattr(self, k).shape) == want, (k, tuple(getattr(self, k).shape), want)
        assert lengths is not None and tuple(lengths.shape) == (n,)
        self.lengths = lengths
        self.longest = int(longest) if longest is not None else int(t)

    def _extra(self) -> dict:
        return {}

    @classmethod
    def concat(cls, parts):
        """The datasets of several episode batches as one (rows concatenated; the parts share the blocking width)."""
        import torch
        parts = list(parts)
        if len(parts) == 1:
            return parts[0]
        T = parts[0].input_ids.shape[1]
        assert all(p.input_ids.shape[1] == T for p in parts), "the parts share the blocking width (pass max_length)"
        assert all(p.fields == parts[0].fields for p in parts)
        extra = {k: torch.cat([p._extra()[k] for p in parts]) for k in parts[0]._extra()}
        return cls(longest=max(p.longest for p in parts), lengths=torch.cat([p.lengths for p in parts]),
                   **{k: torch.cat([getattr(p, k) for p in parts]) for k in parts[0].fields}, **extra)

    def trimmed_width(self, multiple: int = 64) -> int:
        """The narrowest batch width (a multiple of `multiple`) that still holds every row."""
        return min(int(self.input_ids.shape[1]), -(-max(self.longest, 2) // multiple) * multiple)

    def __len__(self) -> int:
        return int(self.input_ids.shape[0])

    def _gather(self, src, index, n):
        import torch
        src2 = src.view(src.shape[0], -1)
        dst = torch.empty((n, src2.shape[1]), dtype=src.dtype, device=src.device)
        _lib.check(_lib.lib().lmrl_gather_rows_bytes(src2.data_ptr(), index.data_ptr(), dst.data_ptr(), n, src2.shape[1] * src2.element_size(),
                                                     _lib.stream_ptr()), "lmrl_gather_rows_bytes")
        return dst if src.dim() == 2 else dst.view(n)

    @staticmethod
    def _mask_pos(lengths, n, w):
        import torch
        am = torch.empty(n, w, dtype=torch.uint8, device=lengths.device)
        pos = torch.empty(n, w, dtype=torch.int32, device=lengths.device)
        _lib.check(_lib.lib().lmrl_len_mask_pos(lengths.data_ptr(), n, w, am.data_ptr(), pos.data_ptr(), _lib.stream_ptr()), "lmrl_len_mask_pos")
        return am, pos

    def _index(self, index):
        """Batch indices as an int32 device tensor (uploaded once per batch)."""
        import torch
        if not isinstance(index, torch.Tensor):
            index = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(self.input_ids.device)
        return index.to(torch.int32).contiguous()

    def batch(self, index, width: Optional[int] = None) -> Dict[str, "torch.Tensor"]:
        """Rows `index` of every array (`lmrl_gather_rows_bytes`) + `attention_mask` / `position_ids` from the rows' lengths
        (`lmrl_len_mask_pos`), keyword-compatible with the trainer's `step`.  width (>= `longest`): keep only the first `width` columns."""
        index = self._index(index)
        n = int(index.numel())
        T = int(self.input_ids.shape[1])
        w = T if width is None else int(width)
        if not (max(self.longest, 2) <= w <= T):
            raise ValueError(f"batch width {w} must lie between the longest row ({self.longest}) and the dataset width ({T})")
        out = {}
        for k in self.fields:
            dst = self._gather(getattr(self, k), index, n)
            if k not in self.ROW:
                cols = w if k in self.WIDE else w - 1
                dst = dst if cols == dst.shape[1] else dst[:, :cols].contiguous()
            out[self.BATCH_NAMES.get(k, k)] = dst
        out["attention_mask"], out["position_ids"] = self._mask_pos(self._gather(self.lengths, index, n), n, w)
        return out

    BATCH_NAMES: dict = {}

    def batches(self, rng, bsize: int, truncate: bool = True, width: Optional[int] = None):
        """One epoch of shuffled batches (`datasets.dataloader` on the device dataset)."""
        n = len(self)
        order = np.arange(n) if rng is None else rng.permutation(n)
        stop = n - (n % bsize) if truncate else n
        for i in range(0, stop, bsize):
            yield self.batch(order[i:i + bsize], width=width)


class DeviceILQLDataset(_DeviceDataset):
    """`ILQLDataset` (ilql/data.py:81-132) resident in HBM: input_ids int32 [N, T], should_take_action uint8 / rewards float32 [N, T-1],
    dones uint8 [N]; on multi-trajectory chains also next_token_ids int32 [N, T], next_dones uint8 [N] (and the next rows' lengths)."""
    FIELDS = ("input_ids", "should_take_action", "rewards", "dones", "next_token_ids", "next_dones")
    WIDE = ("input_ids", "next_token_ids")
    ROW = ("dones", "next_dones")

    def __init__(self, longest=None, lengths=None, next_lengths=None, **arrays):
        super().__init__(longest=longest, lengths=lengths, **arrays)
        self.next_lengths = next_lengths
        assert (self.next_token_ids is None) == (self.next_dones is None) == (next_lengths is None)

    def _extra(self):
        return {} if self.next_lengths is None else dict(next_lengths=self.next_lengths)

    def batch(self, index, width: Optional[int] = None):
        index = self._index(index)
        out = super().batch(index, width)
        out.setdefault("next_token_ids", None)
        out.setdefault("next_dones", None)
        if self.next_lengths is not None:
            n, w = out["next_token_ids"].shape
            out["next_tokens_attention_mask"], out["next_tokens_position_ids"] = self._mask_pos(self._gather(self.next_lengths, index, n), n, w)
        return out

    def to_host(self):
        from .ilql import ILQLDataset
        h = lambda x, dt: None if x is None else x.cpu().numpy().astype(dt)
        return ILQLDataset(h(self.input_ids, np.int32), h(self.should_take_action, np.bool_), h(self.rewards, np.float32), h(self.dones, np.bool_),
                           h(self.next_token_ids, np.int32), h(self.next_dones, np.bool_))


class DeviceMCDataset(_DeviceDataset):
    """`MCDataset` (mc_returns/data.py:76-113) resident in HBM: input_ids int32 [N, T], should_take_action uint8 / returns float32 [N, T-1]."""
    FIELDS = ("input_ids", "should_take_action", "returns")

    def to_host(self) -> Dict[str, np.ndarray]:
        """The dict `MCData.block` returns."""
        return dict(input_ids=self.input_ids.cpu().numpy(), should_take_action=self.should_take_action.cpu().numpy().astype(np.bool_),
                    returns=self.returns.cpu().numpy())


class DeviceMaskDataset(_DeviceDataset):
    """`datasets.MaskDataset` resident in HBM: input_ids int32 / input_training_mask float32 [N, T] (1.0 on action tokens).  A batch names the
    mask `is_action`, the keyword of `GPT2BCTrain.step`."""
    FIELDS = ("input_ids", "input_training_mask")
    WIDE = ("input_ids", "input_training_mask")
    BATCH_NAMES = {"input_training_mask": "is_action"}

    def to_host(self):
        from ..datasets import MaskDataset
        return MaskDataset(self.input_ids.cpu().numpy(), self.input_training_mask.cpu().numpy())


def _longest(blocks) -> int:
    return int(blocks["lengths"].max().item())


def ilql_data_from_records(rec: PPORecords, blocking_strategy: BlockingStrategy, pad_token_id: int, keep=None) -> DeviceILQLDataset:
    """`ILQLData.from_token_trajectory_chain` + `ILQLDataset.from_ilql_data_list` on device records: one row per (kept) trajectory.  Records with
    multi-trajectory chains (Maze, chess) also get `next_token_ids` / `next_dones`; a chain's last trajectory, whose next is None in the
    reference (which then cannot block it next to the others), gets an all-padding next row with next_done = True: no bootstrap."""
    T, left = _strategy(blocking_strategy, rec)
    fields = ["input_ids", "should_take_action", "rewards", "dones"] + (["next_token_ids", "next_dones"] if rec.chain is not None else [])
    b = block_records(rec, T, pad_token_id, left, fields, keep=keep)
    return DeviceILQLDataset(longest=_longest(b), **b)


def record_rtg(rec: PPORecords, gamma: float):
    """Reward-to-go over the action tokens of every UN-truncated record row, scattered to positions of the shifted grid: float32 [n, cap - 1]
    (`lmrl_rtg` on reward[1:] / is_action[1:] with the rows' n_tok - 1 as lengths; mc_returns/data.py:49-74 on single-trajectory chains)."""
    import torch
    if rec.chain is not None:
        raise ValueError("MC returns over multi-trajectory chains are not built on the device")
    if rec.cap < 2:
        raise ValueError("records of one token per row have no shifted grid")
    rw = rec.reward[:, 1:].contiguous()
    sta = rec.is_action[:, 1:].contiguous()
    lens = torch.clamp(rec.n_tok - 1, min=0, max=rec.cap - 1).to(torch.int32).contiguous()
    out = torch.empty_like(rw)
    _lib.check(_lib.lib().lmrl_rtg(_lib.ptr(rw), _lib.ptr(sta), _lib.ptr(lens), _lib.ptr(out), rec.n, rec.cap - 1, float(gamma), _lib.stream_ptr()), "lmrl_rtg")
    return out


def mc_data_from_records(rec: PPORecords, gamma: float, blocking_strategy: BlockingStrategy, pad_token_id: int, keep=None) -> DeviceMCDataset:
    """`MCData.from_token_trajectory_chain(chain, gamma)` + `MCData.block` on device records of single-trajectory chains."""
    rtg = record_rtg(rec, gamma)
    T, left = _strategy(blocking_strategy, rec)
    b = block_records(rec, T, pad_token_id, left, ["input_ids", "should_take_action", "returns"], keep=keep, returns=rtg)
    return DeviceMCDataset(longest=_longest(b), **b)


def mask_data_from_records(rec: PPORecords, blocking_strategy: BlockingStrategy, pad_token_id: int, keep=None) -> DeviceMaskDataset:
    """`MaskDataset.blocked_from_str_segments` with the segments `(text, float(is_action))` of the records' trajectories."""
    T, left = _strategy(blocking_strategy, rec)
    b = block_records(rec, T, pad_token_id, left, ["input_ids", "training_mask"], keep=keep)
    return DeviceMaskDataset(longest=_longest(b), lengths=b["lengths"], input_ids=b["input_ids"], input_training_mask=b["training_mask"])


def record_returns(rec: PPORecords):
    """float32 [n_chains] device tensor: the undiscounted reward sum of every chain (`lmrl_record_returns`)."""
    import torch
    out = torch.empty(rec.n_chains, dtype=torch.float32, device=rec.tokens.device)
    c = rec.c_struct()
    _lib.check(_lib.lib().lmrl_record_returns(ctypes.byref(c), _lib.ptr(out), _lib.stream_ptr()), "lmrl_record_returns")
    return out


def filter_decision(scores, take_top: Optional[float] = None, threshold: Optional[float] = None, top_fraction: Optional[float] = None) -> np.ndarray:
    """Which chains a filter keeps, from their scores alone -> int32 chain indices.
    take_top / threshold: `bc.filter_items` (bc/data.py:32-47) — threshold = np.percentile(scores, 100 - take_top), kept where score >= threshold,
    in data order.  top_fraction: the online filtered-BC loop's rule — `sorted(range(n), key=score, reverse=True)[:int(n * top_fraction)]`, a
    stable sort (equal scores stay in data order), kept in sorted order."""
    if sum(x is not None for x in (take_top, threshold, top_fraction)) != 1:
        raise ValueError("give exactly one of take_top, threshold, top_fraction")
    s = np.asarray(scores, dtype=np.float64)
    if top_fraction is not None:
        order = sorted(range(len(s)), key=lambda i: s[i], reverse=True)
        return np.asarray(order[: int(len(s) * top_fraction)], dtype=np.int32)
    if take_top is not None:
        threshold = np.percentile(s, 100 - take_top)
    return np.flatnonzero(s >= threshold).astype(np.int32)


def filter_records(rec: PPORecords, take_top: Optional[float] = None, threshold: Optional[float] = None, top_fraction: Optional[float] = None):
    """%BC filtering on device records -> `ValidatedKeep` of the kept ROWS (every trajectory of a kept chain, chains in the order
    `filter_decision` gives), to pass as `keep=` to the builders above.  The [n_chains] score vector is read back and the decision made on the
    host; token data stays where it is."""
    import torch
    scores = record_returns(rec).cpu().numpy()
    chains = filter_decision(scores, take_top=take_top, threshold=threshold, top_fraction=top_fraction)
    if rec.chain is None:
        rows = chains
    else:
        chain_h = rec.chain.cpu().numpy()                        # [n] int32 bookkeeping, not token data
        first = np.searchsorted(chain_h, chains, side="left")
        last = np.searchsorted(chain_h, chains, side="right")
        rows = np.concatenate([np.arange(a, b, dtype=np.int32) for a, b in zip(first, last)]) if len(chains) else np.zeros(0, np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    return ValidatedKeep(torch.from_numpy(rows).to(rec.tokens.device), rows, rec)
