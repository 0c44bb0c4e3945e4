"""Reference words of circuit bootstrapping (cufhe_amd_cb_rotate_batch, cufhe_amd_private_keyswitch_batch,
cufhe_amd_circuit_bootstrap_batch), composed from oracle pieces.

oracle/tfhe_oracle_lvl2.c hard-codes mu = 2^61 in its rotation, so the lvl02 rotation is rebuilt here step by step with any constant
test vector: the rotated test vector and the digits of X^abar acc - acc with the roundings of orc2_blind_rotate / accumulate (numpy),
the products digit x key row by orc2_polymul_ntt (exact mod 2^64), then orc2_sample_extract0.  tests/test_circuit_bootstrap.py shows
that this composition reproduces orc2_blind_rotate + orc2_sample_extract0 word for word at mu = 2^61 before anything relies on it at
mu_r.  The private key switch is a numpy gather-sum mod 2^32.  A rotation takes a second or so of CPU: callers keep word cases small
and run them on threads (ctypes releases the GIL).
"""
from concurrent.futures import ThreadPoolExecutor
import os

import numpy as np

import oracle_lib as ol

n, N, N2 = ol.n, ol.N, ol.N2
NBIT2 = 11
L2, BGBIT2 = 4, 9
CB_L, CB_BGBIT = 3, 6
PKS_T, PKS_BASEBIT = 10, 3
PKS_NUMBASE = (1 << PKS_BASEBIT) - 1
PKS_IN = N2 + 1
PKS_KEY_WORDS = 2 * PKS_IN * PKS_T * PKS_NUMBASE * 2 * N          # 587 489 280
TRGSW_WORDS = 2 * CB_L * 2 * N
STEP2 = 2 * L2 * 2 * N2                                            # uint64 words of one lvl02 key step: [row][comp][N2]
M64 = (1 << 64) - 1


def cb_mu(r):
    """the test-vector constant of rotation r: 2^(63 - (r + 1) Bgbit)"""
    return 1 << (63 - (r + 1) * CB_BGBIT)


def _mod_switch(x):
    return int(x) >> (32 - 1 - NBIT2)


def _rotate64(p, e):
    """X^e p in Z_2^64[X]/(X^N2 + 1), 0 <= e < 2 N2, as accumulate reads it: temp = p[(i - e) mod N2], negated where
    (i < e mod N2) xor (e >= N2)"""
    i = np.arange(N2)
    v = p[(i - e) & (N2 - 1)]
    neg = (i < (e & (N2 - 1))) ^ bool(e >> NBIT2)
    return np.where(neg, (np.uint64(0) - v), v)


def _decomp_consts():
    off = 0
    for i in range(1, L2 + 1):
        off += (1 << (BGBIT2 - 1)) << (64 - i * BGBIT2)
    return np.uint64(off & M64), np.uint64(1 << (64 - L2 * BGBIT2 - 1))


def blind_rotate_mu(keys2, tlwe0, mu, steps=n):
    """the accumulator [2][N2] (uint64) of the lvl02 rotation of lvl0 ciphertext tlwe0 with the constant test vector mu"""
    L = keys2.L
    tlwe0 = np.ascontiguousarray(tlwe0, np.uint32)
    bar = 2 * N2 - _mod_switch(tlwe0[n])
    i = np.arange(N2)
    acc = np.zeros(2 * N2, np.uint64)
    if bar == 2 * N2:
        acc[N2:] = np.uint64(mu)
    else:
        neg = (i < (bar & (N2 - 1))) ^ bool(bar >> NBIT2)
        acc[N2:] = np.where(neg, np.uint64((-mu) & M64), np.uint64(mu))
    doff, roff = _decomp_consts()
    ro0 = 1 << (32 - 2 - NBIT2)
    res = np.zeros(N2, np.uint64)
    digits = np.zeros((2 * L2, N2), np.int32)
    with np.errstate(over="ignore"):
        for s in range(steps):
            abar = _mod_switch((int(tlwe0[s]) + ro0) & 0xFFFFFFFF)
            for j in range(2):
                t = _rotate64(acc[j * N2:(j + 1) * N2], abar) - acc[j * N2:(j + 1) * N2] + doff + roff
                for d in range(L2):
                    digits[j * L2 + d] = ((t >> np.uint64(64 - (d + 1) * BGBIT2)) & np.uint64((1 << BGBIT2) - 1)).astype(np.int64) - (1 << (BGBIT2 - 1))
            key = keys2.bk[s * STEP2:(s + 1) * STEP2]
            upd = np.zeros(2 * N2, np.uint64)
            for row in range(2 * L2):
                dr = np.ascontiguousarray(digits[row])
                for out in range(2):
                    L.orc2_polymul_ntt(res, dr, np.ascontiguousarray(key[(row * 2 + out) * N2:(row * 2 + out + 1) * N2]))
                    upd[out * N2:(out + 1) * N2] += res
            acc += upd
    return acc


def sample_extract0(keys2, acc):
    return keys2.sample_extract(acc)


def cb_rotate_one(keys2, tlwe0):
    """stage 1 of one circuit bootstrap: [l][N2 + 1] uint64, mu_r added to b"""
    out = np.zeros((CB_L, PKS_IN), np.uint64)
    for r in range(CB_L):
        out[r] = sample_extract0(keys2, blind_rotate_mu(keys2, tlwe0, cb_mu(r)))
        out[r, N2] += np.uint64(cb_mu(r))
    return out


def cb_rotate_batch(keys2, tlwe0s, threads=None):
    threads = threads or min(16, os.cpu_count() or 1)
    tlwe0s = np.ascontiguousarray(tlwe0s, np.uint32).reshape(-1, n + 1)
    with ThreadPoolExecutor(threads) as ex:
        return np.stack(list(ex.map(lambda g: cb_rotate_one(keys2, tlwe0s[g]), range(tlwe0s.shape[0]))))


def pks_digits(tlwe2):
    """(i, j, v) of the nonzero digits of one lvl2 TLWE: abar_i = tlwe2[i] + 2^33, a_ij = (abar_i >> (64 - 3 (j + 1))) & 7"""
    with np.errstate(over="ignore"):
        abar = np.ascontiguousarray(tlwe2, np.uint64) + np.uint64(1 << (64 - PKS_T * PKS_BASEBIT - 1))
    sh = np.array([64 - PKS_BASEBIT * (j + 1) for j in range(PKS_T)], np.uint64)
    a = ((abar[:, None] >> sh[None, :]) & np.uint64(PKS_NUMBASE)).astype(np.int64)      # [N2 + 1][t]
    ii, jj = np.nonzero(a)
    return ii, jj, a[ii, jj]


def private_keyswitch_one(key, tlwe2):
    """the two TRLWEs [2][2][N] (uint32) of one lvl2 TLWE: 0 - sum K[u][i][j][a_ij - 1] over the nonzero digits"""
    k = key.reshape(2, PKS_IN * PKS_T * PKS_NUMBASE, 2 * N)
    ii, jj, vv = pks_digits(tlwe2)
    idx = (ii * PKS_T + jj) * PKS_NUMBASE + (vv - 1)
    out = np.zeros((2, 2 * N), np.uint32)
    for u in range(2):
        s = k[u][idx].sum(axis=0, dtype=np.uint64)
        out[u] = ((np.uint64(0) - s) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out.reshape(2, 2, N)


def private_keyswitch_batch(key, tlwe2s, threads=None):
    threads = threads or min(16, os.cpu_count() or 1)
    tlwe2s = np.ascontiguousarray(tlwe2s, np.uint64).reshape(-1, PKS_IN)
    with ThreadPoolExecutor(threads) as ex:
        return np.stack(list(ex.map(lambda g: private_keyswitch_one(key, tlwe2s[g]), range(tlwe2s.shape[0]))))


def trgsw_from_stage1(key, stage1):
    """[count][l][N2 + 1] (stage 1) -> the TRGSWs [count][(k+1) l][k+1][N]: row c l + r = PrivKS_c(tlwe2_r)"""
    stage1 = np.asarray(stage1, np.uint64)
    count = stage1.shape[0]
    p = private_keyswitch_batch(key, stage1.reshape(-1, PKS_IN)).reshape(count, CB_L, 2, 2, N)
    return np.ascontiguousarray(p.transpose(0, 2, 1, 3, 4)).reshape(count, 2 * CB_L, 2, N)
