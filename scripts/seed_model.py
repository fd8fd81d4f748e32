#!/usr/bin/env python3
"""CPU model of the int8 filter's seeded thresholds (DESIGN.md "Seeded thresholds"): an estimate,
not a measurement.

One wave's 64 queries against one cold piece of workload A (uniform rows in [-1, 1), d = 128,
k = 10, int8 operands with s = 1 / 127): the k-th largest of the 32 group maxima of
a = nq . nt - n_r over a strided sample of S rows gives the seed U(a_k) (knn_i8_seed_bound's
formula with a Cauchy-Schwarz band), and the model reports

  * whether every seed is >= the exact k-th distance of the piece (it must be),
  * seed / D_(k), and how many of the piece's rows lie under the seed (the rows the filter still
    has to keep: every one of them passes the exact test L <= thr at the start of the piece),
  * the rows a threshold that starts at +inf keeps over the same piece (the k-th smallest U seen
    so far: per tile over the dense start, then every 64 tiles as the kernel's flush does)
    against the rows kept when it starts at the seed.

usage: python scripts/seed_model.py [--rows 333312] [--sample 8192 16384 32768 65536] [--k 10]
"""
import argparse

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=333_312, help="rows of the piece (a third of A)")
    ap.add_argument("--sample", type=int, nargs="+", default=[8192, 16384, 32768, 65536])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    d, k, s = 128, a.k, np.float32(1 / 127)
    s2 = np.float32(2) * s * s
    q = rng.uniform(-1, 1, (a.queries, d)).astype(np.float32)
    iq = np.clip(np.rint(q / s), -127, 127).astype(np.int32)
    qn = (q.astype(np.float64) ** 2).sum(1)
    coef = (9 * d + 512) * 2.0 ** -24

    def block(n):
        """n fresh train rows: (exact distances, accumulator values a, tn, |t - rt|, |rt|)."""
        t = rng.uniform(-1, 1, (n, d)).astype(np.float32)
        it = np.clip(np.rint(t / s), -127, 127).astype(np.int32)
        tn = (t.astype(np.float64) ** 2).sum(1)
        n_r = np.floor(tn / s2).astype(np.int64)
        D = qn[:, None] + tn[None, :] - 2.0 * (q.astype(np.float64) @ t.astype(np.float64).T)
        acc = iq.astype(np.int64) @ it.T.astype(np.int64) - n_r[None, :]
        rt = it * np.float64(s)
        return D, acc, tn, np.sqrt(((t - rt) ** 2).sum(1)), np.sqrt((rt ** 2).sum(1))

    # the piece, in chunks of 8192 rows; the statistics' maxima over it stand for the train set's
    Ds, As, st = [], [], np.zeros(3)
    for r0 in range(0, a.rows, 8192):
        D, acc, tn, e, m = block(min(8192, a.rows - r0))
        Ds.append(D.astype(np.float32)); As.append(acc.astype(np.int32))
        st = np.maximum(st, [tn.max(), e.max(), m.max()])
    D, A = np.concatenate(Ds, 1), np.concatenate(As, 1)
    qe = np.sqrt(((q - iq * np.float64(s)) ** 2).sum(1))
    dl = coef * (qn + st[0]) + 2 * (np.sqrt(qn) * st[1] + qe * st[2]) + s2   # band with the global maxima
    U = qn[:, None] - np.float64(s2) * A + dl[:, None]
    L = qn[:, None] - np.float64(s2) * A - dl[:, None]
    dk = np.sort(D, 1)[:, k - 1]

    def kept(start):
        """Rows kept over the piece by a threshold that starts at `start` (per query) and drops to
        the k-th smallest U of the kept rows (per tile at first, then every 64 tiles)."""
        thr, n = start.copy(), np.zeros(len(start), np.int64)
        best = np.full((len(start), k), np.inf)
        c0 = 0
        while c0 < D.shape[1]:
            w = 32 if c0 < 8192 else 2048  # (the dense start visits tile by tile; later passes wait for a flush)
            keep = L[:, c0:c0 + w] <= thr[:, None]
            n += keep.sum(1)
            best = np.sort(np.concatenate([best, np.where(keep, U[:, c0:c0 + w], np.inf)], 1), 1)[:, :k]
            thr = np.minimum(thr, best[:, k - 1])
            c0 += w
        return n

    cold = kept(np.full(a.queries, np.inf))
    print(f"piece of {a.rows} rows, {a.queries} queries, k = {k}: unseeded keeps {cold.mean():.0f} rows per query")
    for S in a.sample:
        # the sample: S fresh rows of the same distribution (the strided sample of the whole train
        # set); the group of a sampled row is its place in its 32-row tile
        Dm, Am, *_ = block(S)
        gmax = Am.reshape(a.queries, S // 32, 32).max(1)
        ak = np.sort(gmax, 1)[:, -k]
        seed = qn - np.float64(s2) * ak + dl
        dk_all = np.minimum(dk, np.sort(Dm, 1)[:, k - 1])  # (the train set holds the sample too)
        under = (L <= seed[:, None]).sum(1)
        print(f"S = {S:6d}: valid {bool(np.all(seed >= dk_all))}  seed / D_(k) median {np.median(seed / dk):.3f}  "
              f"rows of the piece under the seed {under.mean():.0f}  kept with the seed {kept(seed).mean():.0f}")


if __name__ == "__main__":
    main()
