"""predict_chain against the loop of single predictions (the reference's average / particles caller pattern,
g3py/bayesian/models.py:489-543): SE + noise, d = 4, M = 256 query points, a chain of up to 4096 hyper-parameter rows.

    python scripts/predict_chain_bench.py                 # every N: predict_chain, its phases and transfers, logp_chain, the loop
    python scripts/predict_chain_bench.py --loop-only     # only the loop of single predict calls (runs on a tree without
                                                          # predict_chain: the figure of the parent commit)
One JSON line per N on stdout.  Times are medians over --reps calls after one warm-up call (wall clock around calls that
return host arrays, so each includes its synchronisation)."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import g3py_amd as g3
from g3py_amd import _lib


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loop-only', action='store_true')
    ap.add_argument('--sizes', default='64,128,256,512,1024')
    ap.add_argument('--members', type=int, default=4096)
    ap.add_argument('--loop-rows', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    d, M = 4, 256
    for N in [int(v) for v in a.sizes.split(',')]:
        rng = np.random.default_rng(N)
        X = rng.uniform(0, N ** (1 / d), (N, d))
        y = np.sin(X.sum(1) / 2) + 0.1 * rng.standard_normal(N)
        S = rng.uniform(0, N ** (1 / d), (M, d))
        gp = g3.GaussianProcess(space=S, location=g3.Zero(), kernel=g3.SE(X))
        gp.observed(X, y)
        p = gp.params_test
        by = {v.name: v for v in gp.model.vars}
        for k, val in dict(GP_SE_var=1.0, GP_SE_rate=np.ones(d), GP_Noise_var=0.1).items():
            p[by[k].key] = np.log(val) * np.ones(by[k].shape)
        a0 = gp.active.dict_to_array(p)
        Np = _lib.roundup(N)
        per = ((Np + 128) * Np + Np * 128 + Np + 3 * M) * 8
        B = max(1, min(a.members, int((4e9 - 2 ** 28) // per)))
        chain = a0 + 0.1 * rng.standard_normal((B, len(a0)))
        rows = chain[:min(a.loop_rows, B)]
        out = dict(N=N, M=M, d=d, members=B)

        def loop():
            for r in rows:
                gp.predict(gp.active.array_to_dict(r), var=True)
        ms = median_ms(loop, max(2, a.reps // 2))
        out.update(loop_rows=len(rows), loop_ms_per_row=ms / len(rows), loop_rows_per_s=1e3 * len(rows) / ms)
        if not a.loop_only:
            ms = median_ms(lambda: gp.predict_chain(chain, var=True), a.reps)
            out.update(predict_chain_ms=ms, predict_chain_rows_per_s=1e3 * B / ms, predict_chain_ms_per_row=ms / B,
                       speedup_per_row_vs_loop=out['loop_ms_per_row'] / (ms / B))
            ms = median_ms(lambda: gp.logp_chain(chain), a.reps)
            out.update(logp_chain_ms=ms, logp_chain_rows_per_s=1e3 * B / ms)
            dev = gp.device
            dev.prof_enable(2)
            dev.prof_reset()
            gp.predict_chain(chain, var=True)
            pr = dev.prof_collect()
            dev.prof_enable(0)
            ph = dict(factor=pr['gram']['ms'] + pr['potrf']['ms'], cross_gram=pr['cross_gram']['ms'], solve=pr['trsm']['ms'])
            tot = sum(ph.values()) or 1.0
            out.update(device_ms={k: round(v, 4) for k, v in ph.items()}, device_share={k: round(v / tot, 3) for k, v in ph.items()})
            # the call's host traffic on its own: the (members, N) deltas up, three (members, roundup(M, 128)) results down
            Mp = _lib.roundup(M, _lib.G3_RHS_PAD)
            delta = np.zeros((B, N))

            def up():
                dev.upload(delta).free()
            res = dev.alloc(B, Mp, np.float64)
            out.update(host_ms=dict(delta_upload=round(median_ms(up, a.reps), 4),
                                    results_download=round(median_ms(lambda: [dev.download(res, B, M) for _ in range(3)], a.reps), 4)))
            res.free()
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
