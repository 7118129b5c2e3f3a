"""include/gigapose_appear.h restated in numpy and Python integers: what libgigapose_appear.so (gigapose_amd/appearance.py) is held
to bit for bit (tests/test_gpu_appear.py), and what tests/test_appear_host.py holds to readings that cannot share its mistakes.

  chain_sum(v)                                 SUM of the header: four strided chains, (S0 + S1) + (S2 + S3)
  quantised(x, gamma, beta, eps)               tokens (.., C) -> (q int32, status): float64 in the header's order, numpy.sqrt
  q_to_limbs(q) / limbs_to_q(a)                the balanced base-128 digits and back
  patch_descriptors(x, gamma, beta, eps)       (B, 256, C) tokens -> (a int8 (3, B, 256, C), status int32 (B, 256))
  patch_valid(mask, num, den)                  (B, 224, 224) f32 -> (valid u8 (B, 256), count int32 (B), set u8 (B, 256))
  dots(qa, ta)                                 limbs (3, 256, C) x (3, 256, C) -> dot (256, 256) int64, exact
  appearance(qa, q_valid, ta, t_valid, qi, ti) -> dict(sum, n, status, best, arg)
`variant` names a subtly wrong version (VARIANTS); the host tests show that each of them fails a check."""
import numpy as np

Q_BITS = 20
Q_ONE = 1 << Q_BITS
PATCHES, CELL, SIDE = 256, 14, 16
NON_FINITE, ZERO_NORM = 1, 2
BAD_INDEX, NO_QUERY_PATCH, NO_TEMPLATE_PATCH = 1, 2, 4
VARIANTS = ("max_over_all", "mean_over_all", "last_maximum", "max_from_zero", "truncate", "unbalanced", "swapped")


# ------------------------------------------------------------------------------------------------ descriptors
def chain_sum(v):
    """SUM of the header over the last axis of v (.., C) float64: S_j adds v[j], v[j + 4], .. in order to +0.0; (S0 + S1) + (S2 + S3)."""
    v = np.asarray(v, np.float64)
    S = np.zeros(v.shape[:-1] + (4,), np.float64)
    for c0 in range(0, v.shape[-1], 4):
        n = min(4, v.shape[-1] - c0)
        S[..., :n] = S[..., :n] + v[..., c0:c0 + n]
    return (S[..., 0] + S[..., 1]) + (S[..., 2] + S[..., 3])


def quantised(x, gamma, beta, eps, variant=None):
    """x (.., C) f32 tokens -> (q int32 (.., C), status int32 (..))."""
    x = np.asarray(x, np.float32).astype(np.float64)
    g, b = np.asarray(gamma, np.float32).astype(np.float64), np.asarray(beta, np.float32).astype(np.float64)
    C = np.float64(x.shape[-1])
    with np.errstate(all="ignore"):
        mean = chain_sum(x) / C
        dev = x - mean[..., None]
        var = chain_sum(dev * dev) / C
        r = np.float64(1.0) / np.sqrt(var + np.float64(eps))
        y = (dev * r[..., None]) * g + b
        n2 = chain_sum(y * y)
        status = np.zeros(x.shape[:-1], np.int32)
        status[n2 == 0] = ZERO_NORM
        status[~np.isfinite(x).all(axis=-1) | ~np.isfinite(n2)] = NON_FINITE
        norm = np.where(status != 0, 1.0, np.sqrt(n2))
        scaled = (y / norm[..., None]) * np.float64(Q_ONE)
        scaled[status != 0] = 0.0
        q = np.trunc(scaled) if variant == "truncate" else np.rint(scaled)
    return q.astype(np.int32), status


def q_to_limbs(q, variant=None):
    """q integers (..) within 2^20 -> a int8 (3, ..): a0 = ((q + 64) mod 128) - 64, q1 = (q - a0) / 128, a1 likewise, a2 = (q1 - a1) / 128.
    The wrong version takes digits in [0, 127] (int16: they still fit an int8 -- except the top one of a negative q, which is what breaks)."""
    q = np.asarray(q, np.int64)
    if variant == "unbalanced":
        a0 = q % 128
        q1 = (q - a0) // 128
        a1 = q1 % 128
        return np.stack([a0, a1, (q1 - a1) // 128]).astype(np.int16)
    a0 = (q + 64) % 128 - 64
    q1 = (q - a0) // 128
    a1 = (q1 + 64) % 128 - 64
    return np.stack([a0, a1, (q1 - a1) // 128]).astype(np.int8)


def limbs_to_q(a):
    """a (3, ..) -> q int32 (..) = a0 + 128 a1 + 16384 a2."""
    a = np.asarray(a).astype(np.int64)
    return (a[0] + 128 * a[1] + 16384 * a[2]).astype(np.int32)


def patch_descriptors(x, gamma, beta, eps, variant=None):
    """x (B, 256, C) f32: the patch tokens (the class token already dropped) -> (a int8 (3, B, 256, C), status int32 (B, 256))."""
    q, status = quantised(x, gamma, beta, eps, variant)
    return q_to_limbs(q, variant), status


# ------------------------------------------------------------------------------------------------ occupancy
def patch_valid(mask, num, den):
    """mask (B, 224, 224) f32 -> (valid u8 (B, 256), count int32 (B), set u8 (B, 256)): one patch at a time."""
    mask = np.asarray(mask, np.float32)
    B = mask.shape[0]
    half = np.float32(0.5)
    valid, sets = np.zeros((B, PATCHES), np.uint8), np.zeros((B, PATCHES), np.uint8)
    for b in range(B):
        for n in range(PATCHES):
            py, px = divmod(n, SIDE)
            with np.errstate(invalid="ignore"):
                k = int((mask[b, CELL * py:CELL * py + CELL, CELL * px:CELL * px + CELL] > half).sum())
            sets[b, n] = k
            valid[b, n] = 1 if k * int(den) > int(num) * CELL * CELL else 0
    return valid, valid.sum(axis=1).astype(np.int32), sets


# ------------------------------------------------------------------------------------------------ appearance
def dots(qa, ta):
    """qa, ta (3, 256, C) limbs -> dot (256, 256) int64: [i, j] = sum_c q_query[i, c] * q_bank[j, c], exact in int64."""
    q, t = limbs_to_q(qa).astype(np.int64), limbs_to_q(ta).astype(np.int64)
    bound = int(np.abs(q).max(initial=0)) * int(np.abs(t).max(initial=0)) * q.shape[-1]
    if bound >= 1 << 53:
        return q @ t.T
    # every product and every partial sum is an integer below 2^53: the float64 product (BLAS, any order) is exact
    return (q.astype(np.float64) @ t.astype(np.float64).T).astype(np.int64)


def limb_sums(a, b):
    """a, b (3, C) limbs of one patch each -> [s0 .. s4] Python integers, s_w = sum over c and u + v = w of a_u[c] * b_v[c]: what the five
    int32 accumulators hold; dot = s0 + (s1 << 7) + (s2 << 14) + (s3 << 21) + (s4 << 28)."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    return [sum(int((a[u] * b[w - u]).sum()) for u in range(3) if 0 <= w - u < 3) for w in range(5)]


def combine(s):
    return s[0] + (s[1] << 7) + (s[2] << 14) + (s[3] << 21) + (s[4] << 28)


def appearance(qa, q_valid, ta, t_valid, qi, ti, variant=None):
    """qa (3, Bq, 256, C), q_valid (Bq, 256), ta (3, R, 256, C), t_valid (R, 256), qi, ti (P)
    -> dict(sum int64 (P), n int32 (P), status int32 (P), best int64 (P, 256), arg int32 (P, 256))."""
    qa, ta = np.asarray(qa), np.asarray(ta)
    q_valid, t_valid = np.asarray(q_valid) != 0, np.asarray(t_valid) != 0
    Bq, R, P = qa.shape[1], ta.shape[1], len(qi)
    out = dict(sum=np.zeros(P, np.int64), n=np.zeros(P, np.int32), status=np.zeros(P, np.int32), best=np.zeros((P, PATCHES), np.int64),
               arg=np.full((P, PATCHES), -1, np.int32))
    for p in range(P):
        q, t = int(qi[p]), int(ti[p])
        if not (0 <= q < Bq and 0 <= t < R):
            out["status"][p] = BAD_INDEX
            continue
        qv, tv = q_valid[q], t_valid[t]
        if variant == "max_over_all":
            tv = np.ones_like(tv)
        out["status"][p] = (0 if qv.any() else NO_QUERY_PATCH) | (0 if tv.any() else NO_TEMPLATE_PATCH)
        if out["status"][p]:
            continue
        dot = dots(ta[:, t], qa[:, q]) if variant == "swapped" else dots(qa[:, q], ta[:, t])
        rows = np.arange(PATCHES) if variant == "mean_over_all" else np.flatnonzero(qv)
        cols = np.flatnonzero(tv)
        sub = dot[np.ix_(rows, cols)]
        if variant == "max_from_zero":
            sub = np.maximum(sub, 0)
        at = sub.shape[1] - 1 - np.argmax(sub[:, ::-1], axis=1) if variant == "last_maximum" else np.argmax(sub, axis=1)      # argmax: the first
        out["best"][p, rows], out["arg"][p, rows] = sub[np.arange(len(rows)), at], cols[at]
        out["sum"][p], out["n"][p] = out["best"][p].sum(), len(rows)
    return out


def float_appearance(total, n):
    """sum / (n * 2^40) in float64, one correctly rounded division (both operands are exact doubles); n = 0 gives 0."""
    total, n = np.asarray(total, np.int64).astype(np.float64), np.asarray(n, np.int64).astype(np.float64)
    return np.where(n > 0, total / (np.maximum(n, 1.0) * np.float64(1 << (2 * Q_BITS))), 0.0)
