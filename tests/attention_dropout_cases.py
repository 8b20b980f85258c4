"""The mask contract of sn_set_attention_drop_f32 / sn_set_attention_drop_bwd_f32 (include/signnet_hip.h) restated in numpy.

    w      = philox4x32_10(counter = (lo32(n*H + h), (q << 16) | (key >> 2), site, lo32(step)), key = (lo32(seed), hi32(seed)))
    keep   = w[key & 3] >= floor(p * 2^32)
    factor = keep ? float32(1/(1-p)) : 0            multiplies P[n, h, q, key] after the softmax
    site   = 0x41540000 + index of the rho layer

Neither N nor K enters.  The generator, the threshold and the scale are those of tests/dropout_cases.py (Philox4x32-10 pinned to the
Random123 known answers by tests/test_dropout_cases_cpu.py).  Pure numpy: no GPU, no torch.
"""
import numpy as np

from dropout_cases import MASK32, philox4x32_10, scale_of, threshold_of

SITE0 = 0x41540000           # + index of the rho layer
P_TINY = 2.0 ** -33          # threshold 0: keeps everything
PS = [0.1, 0.25, 0.9]
SEED, STEP = 0x1234_5678_9ABC_DEF1, 41


def words(N, H, K, seed, step, site):
    """uint32 [N, H, K, K]: the word of every (node, head, query, key) element."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    row = np.arange(N * H, dtype=np.uint64).reshape(N * H, 1, 1)
    q = np.arange(K, dtype=np.uint64).reshape(1, K, 1)
    kg = np.arange((K + 3) // 4, dtype=np.uint64).reshape(1, 1, -1)
    w = philox4x32_10((row & np.uint64(MASK32), (q << np.uint64(16)) | kg, int(site) & MASK32, int(step) & MASK32),
                      (seed & MASK32, seed >> 32))
    return np.stack(w, axis=-1).reshape(N * H, K, -1)[:, :, :K].reshape(N, H, K, K)


def keep_mask(N, H, K, p, seed, step, site):
    """bool [N, H, K, K]: the elements the attention kernels keep."""
    return words(N, H, K, seed, step, site) >= np.uint32(threshold_of(p))


def factors(N, H, K, p, seed, step, site):
    """float32 [N, H, K, K]: 0 or float32(1/(1-p)) — what an explicit prob_mask of the same dropout holds."""
    return np.where(keep_mask(N, H, K, p, seed, step, site), scale_of(p), np.float32(0.0)).astype(np.float32)
