"""float32 numpy restatement of the parallel one-sided Jacobi of csrc/evd.hip / csrc/evd_large.hip: round-robin
tournament of disjoint column pairs on G = L V, Rutishauser rotation with the three-transcendental parameters, rotate while
|g_i.g_j| > thr |g_i||g_j|, columns below 1e-6 of the largest norm left alone, Rayleigh quotients, ascending order.
numpy's own tournament and summation order: it shows what the METHOD reaches in float32, not the kernel's bits."""
import numpy as np

f32 = np.float32


def pairs(m, step):
    idx = [(step + i) % (m - 1) for i in range(m - 1)] + [m - 1]
    return np.array([idx[i] for i in range(m // 2)]), np.array([idx[m - 1 - i] for i in range(m // 2)])


def jacobi(L, thr=5e-7, max_sweeps=30):
    """Returns (eigenvalues ascending, eigenvectors as columns, sweeps run)."""
    n = L.shape[0]
    m = n + (n & 1)
    G = np.zeros((n, m), f32)
    V = np.zeros((n, m), f32)
    G[:, :n] = L.astype(f32)
    V[:, :n] = np.eye(n, dtype=f32)
    big2 = f32(max(float((G * G).sum(0, dtype=f32).max()), 1e-30))
    sweeps = 0
    for sweep in range(max_sweeps):
        rotated = 0
        for step in range(m - 1):
            i, j = pairs(m, step)
            gi, gj = G[:, i], G[:, j]
            a = (gi * gi).sum(0, dtype=f32)
            b = (gj * gj).sum(0, dtype=f32)
            g = (gi * gj).sum(0, dtype=f32)
            live = np.minimum(a, b) > f32(1e-12) * big2
            rot = live & (g * g > f32(thr) * f32(thr) * (a * b))
            if not rot.any():
                continue
            rotated += int(rot.sum())
            d = (b - a) * f32(0.5)
            R = np.sqrt(d * d + g * g)
            with np.errstate(divide="ignore", invalid="ignore"):
                w = f32(1) / np.sqrt(f32(2) * R * (R + np.abs(d)))
                c = (R + np.abs(d)) * w
                s = np.where(d >= 0, f32(1), f32(-1)) * g * w
            c = np.where(rot, c, f32(1)).astype(f32)
            s = np.where(rot, s, f32(0)).astype(f32)
            tau = (s / (f32(1) + c)).astype(f32)
            for M in (G, V):
                x, y = M[:, i].copy(), M[:, j].copy()
                M[:, i] = x - s * (y + tau * x)
                M[:, j] = y + s * (x - tau * y)
        sweeps = sweep + 1
        if rotated == 0:
            break
    lam = (V[:, :n] * G[:, :n]).sum(0, dtype=f32)
    order = np.argsort(lam, kind="stable")
    return lam[order], V[:, :n][:, order], sweeps
