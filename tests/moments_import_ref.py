"""The consistency check of ssx_spectral_moments_import (include/ssx.h) restated in numpy: what a Q must satisfy against the S and N it is imported next to.  The
rules hold exactly for everything ssx_spectral_moment_kernel can produce -- Q += (double)f * (double)f from +0.0, the product of two binary32 values exact in
binary64 -- so there is nothing inexact in them.  TEST INFRASTRUCTURE, shared by tests/test_moments_checkpoint_cpu.py and tests/test_moments_checkpoint_gpu.py."""
import numpy as np

RULES = ("n == 0", "n == 1", "n >= 2")     # the words the library names a broken rule by


def violations(S, Q, N, mask=None):
    """S, Q float64 [H, W, B], N uint32 [H, W, B / 4], mask bool [H, W] (the pixels the importing context owns; None: all) -> three bool arrays [H, W, B], where
    each rule is broken, with n = N[..., b % M]:
        n == 0 :  Q is +0.0, bit for bit
        n == 1 :  Q == S * S, or both are NaN
        n >= 2 :  !(Q < 0.0)"""
    S, Q = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    n = np.tile(np.asarray(N), (1, 1, 4))
    own = np.ones(S.shape[:2], dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    own = np.broadcast_to(own[..., None], S.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        ss = S * S
        r0 = (n == 0) & (Q.view(np.uint64) != 0)
        r1 = (n == 1) & ~((Q == ss) | (np.isnan(Q) & np.isnan(ss)))
        r2 = (n >= 2) & (Q < 0.0)
    return r0 & own, r1 & own, r2 & own


def broken_rule(S, Q, N, mask=None):
    """The first rule (0, 1, 2: an index into RULES) some owned pixel breaks -- what the library reports -- or None: the import is accepted."""
    for k, bad in enumerate(violations(S, Q, N, mask)):
        if bad.any():
            return k
    return None
