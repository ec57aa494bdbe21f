"""The opt-in deterministic mode: the training step gives the same bits on every run (one process, one GPU, same build, same inputs
and seed).  DESIGN.md, "Deterministic mode", lists what the mode switches; the default path is untouched.

Initialised from the environment variable ESVIT_DETERMINISTIC (1 / 0) at import; ``esvit_amd.set_deterministic`` switches it later.
"""
import os

_ENV = os.environ.get("ESVIT_DETERMINISTIC", "0")
if _ENV not in ("0", "1"):
    raise ValueError("ESVIT_DETERMINISTIC: 1 or 0, not %r" % _ENV)
_ON = _ENV == "1"


def set_deterministic(on):
    """Switch the deterministic mode: ordered table gradients and norm statistics (no float atomics), the matrix route for every
    resampled ViT position embedding.  Takes effect at the next forward / update; an updater built earlier regrows its buffer."""
    global _ON
    if not isinstance(on, (bool, int)) or on not in (0, 1):
        raise ValueError("set_deterministic: True or False, not %r" % (on,))
    _ON = bool(on)


def is_deterministic():
    return _ON
