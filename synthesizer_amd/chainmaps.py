"""
Chain maps: the reference mixer's saturating chain over a range of voices, as a value (host arithmetic, numpy).

Upstream mixes int16 voices with ``mixed = audioop.add(mixed, voice, 2)`` down the voices in order.  For one int16 value that
chain over a RANGE of voices is the map ``x -> clamp(x + add, lo, hi)``, and such maps compose in order -- so the chain over a
whole table is the composition of the maps of its consecutive ranges (banks, voice shards on several GPUs), applied to silence.

Wire format (include/synthhip.h, ``sh_chain_map``): 8 bytes per value, ``int32 add; int16 lo; int16 hi`` -- ``CHAIN_MAP_DTYPE``.
A mono block has ``nframes`` maps, a stereo block ``2 * nframes``, interleaved L / R like its samples.

``add`` saturates at +-``ADD_MAX`` (2^17): once ``|add| >= 65535`` every int16 ``x`` already lands on ``lo`` or ``hi``
(``x + add >= -32768 + 65535 = 32767 >= hi``, and the mirror image), so the map on int16 inputs is unchanged, and a sum of two
saturated values stays far inside int32 whatever the number of voices or parts.

The library's kernels (``sh_chain_parts_compose`` / ``_apply``, the ``_parts`` mixdowns) do the same arithmetic on the device;
this module is the statement they are tested against, and what a CPU backend of ``dist.DistVoiceBank`` uses.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

__all__ = ["CHAIN_MAP_DTYPE", "ADD_MAX", "identity", "voice_maps", "compose", "compose_all", "apply", "from_bytes"]

CHAIN_MAP_DTYPE = np.dtype([("add", "<i4"), ("lo", "<i2"), ("hi", "<i2")])
ADD_MAX = 1 << 17


def _sat(a: np.ndarray) -> np.ndarray:
    return np.clip(a, -ADD_MAX, ADD_MAX)


def _pack(add, lo, hi) -> np.ndarray:
    out = np.empty(np.shape(add), dtype=CHAIN_MAP_DTYPE)
    out["add"] = _sat(np.asarray(add, dtype=np.int64))
    out["lo"] = lo
    out["hi"] = hi
    return out


def identity(nvalues: int) -> np.ndarray:
    """The map of no voices: (0, -32768, 32767)."""
    return _pack(np.zeros(nvalues, dtype=np.int64), -32768, 32767)


def voice_maps(samples) -> np.ndarray:
    """The map of one voice's int16 samples: x -> clamp(x + s, -32768, 32767)."""
    s = np.asarray(samples, dtype=np.int16).astype(np.int64)
    return _pack(s, -32768, 32767)


def from_bytes(data: bytes) -> np.ndarray:
    return np.frombuffer(data, dtype=CHAIN_MAP_DTYPE).copy()


def compose(f: np.ndarray, g: np.ndarray) -> np.ndarray:
    """f, then g: (a1 + a2, clamp(lo1 + a2, lo2, hi2), clamp(hi1 + a2, lo2, hi2))."""
    a1, a2 = _sat(f["add"].astype(np.int64)), _sat(g["add"].astype(np.int64))
    lo2, hi2 = g["lo"].astype(np.int64), g["hi"].astype(np.int64)
    lo = np.clip(f["lo"].astype(np.int64) + a2, lo2, hi2)
    hi = np.clip(f["hi"].astype(np.int64) + a2, lo2, hi2)
    return _pack(a1 + a2, lo, hi)


def compose_all(parts: Sequence[np.ndarray], nvalues: Optional[int] = None) -> np.ndarray:
    """The maps of consecutive ranges, in order, folded into one (no parts: the identity)."""
    if not len(parts):
        if nvalues is None:
            raise ValueError("compose_all of no parts needs nvalues")
        return identity(nvalues)
    out = identity(len(parts[0]))                    # (from the identity, as the kernels fold: the same spelling, byte for byte)
    for p in parts:
        out = compose(out, np.asarray(p, dtype=CHAIN_MAP_DTYPE))
    return out


def apply(parts: Sequence[np.ndarray], x0=None, nvalues: Optional[int] = None) -> np.ndarray:
    """The maps of consecutive ranges applied in order to x0 (int16; None: silence) -> int16: the chain's result."""
    if nvalues is None:
        nvalues = len(parts[0]) if len(parts) else len(x0)
    x = np.zeros(nvalues, dtype=np.int64) if x0 is None else np.asarray(x0, dtype=np.int16).astype(np.int64)
    for p in parts:
        p = np.asarray(p, dtype=CHAIN_MAP_DTYPE)
        x = np.clip(x + _sat(p["add"].astype(np.int64)), p["lo"].astype(np.int64), p["hi"].astype(np.int64))
    return x.astype(np.int16)
