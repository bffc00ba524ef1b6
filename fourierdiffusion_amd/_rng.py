"""Philox stream bookkeeping for the engine's on-device noise.

The reference draws from torch's global generator (seeded once by ``torch.manual_seed(cfg.random_seed)``,
cmd/train.py:22, cmd/sample.py:22).  Bit-matching torch's CPU/GPU normal generators on the device is
pointless, so the engine owns a counter-based Philox4x32-10 stream -- but it stays slaved to
torch's generator: every engine call that needs noise draws ONE 62-bit key from torch's global CPU
generator (host-side plumbing) and uses counters [rank_base, rank_base + n/4) under that key.
``torch.manual_seed(s)`` therefore reproduces a run exactly as it does for the reference, and
data-parallel ranks (same seed) get disjoint counter ranges through ``set_rank``.

Counter ranges under one key (offsets relative to the rank's base, ``rank << 56``):
  perturbation / prior / step noise   [0, n / 4) of the call's own key (one key per call)
  resampling uniforms (conditioning="smc")  behind the predictor noise of the same call: with N steps of B rows (n = B / K series)
                                      the uniform of (stage j, series q), j = 0 .. N, is ((word >> 8) + 0.5) / 2^24 of word
                                      (j n + q) % 4 of counter N ceil(B T C / 4) + (j n + q) / 4 (fd_sampler_run_impute_smc)
  dropout site s of encoder layer l   [(4 l + s) << 40, (4 l + s + 1) << 40) of the training call's key (fd_dropout_site_offset)
  label dropout (class conditioning)  [0xFFFF << 40, 0xFFFF << 40 + B / 4] of the same training call's key: the window of "layer
                                      16383, site 3", which no encoder layer reaches; label b is lane b % 4 of counter b / 4
"""
from __future__ import annotations

import torch

_state = {"rank_base": 0, "keys_drawn": 0}


def set_rank(rank: int) -> None:
    """Ranks share the seed; rank r draws counters starting at r << 56."""
    _state["rank_base"] = (int(rank) & 0xFF) << 56


def next_key() -> int:
    """A fresh Philox key from torch's global CPU generator."""
    _state["keys_drawn"] += 1
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item())


def base_offset() -> int:
    return _state["rank_base"]


def stream():
    """(key, offset) for one engine call."""
    return next_key(), _state["rank_base"]


def keys_drawn() -> int:
    """Keys drawn so far in this process (the Trainer measures how many a training step takes, so that a rank whose slice of
    a global batch is empty can discard as many and keep torch's generator in step with the other ranks)."""
    return _state["keys_drawn"]


def set_keys_drawn(n: int) -> None:
    """Put the counter back next to a restored torch generator state (the Trainer's second validation pass)."""
    _state["keys_drawn"] = int(n)


def discard_keys(n: int) -> None:
    for _ in range(int(n)):
        next_key()
