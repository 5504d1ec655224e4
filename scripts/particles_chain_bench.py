"""particles (one joint posterior draw per chain row, batched) against the loop of single sample calls (the reference's
particles caller pattern, g3py/bayesian/models.py:521-543): SE + noise, d = 4, fp64, N = M, one draw per row, a chain of
4096 hyper-parameter rows.

    python scripts/particles_chain_bench.py                 # every size: particles, its device phases, the retry share, the loop
    python scripts/particles_chain_bench.py --loop-only     # only the loop of gp.sample(row) calls (runs on a tree without
                                                            # particles: the figure of the parent commit)
    python scripts/particles_chain_bench.py --batched-only --sizes 128 --reps 2
                                                            # identical particles calls only (1 warm-up + reps): for a
                                                            # rocprofv3 --kernel-trace --stats run, kernel time / (reps + 1) per call
One JSON line per size on stdout.  Times are medians over --reps calls after one warm-up call (wall clock around calls that
return host arrays, so each includes its synchronisation)."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import g3py_amd as g3


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
    ap.add_argument('--batched-only', action='store_true')
    ap.add_argument('--sizes', default='128,256')
    ap.add_argument('--members', type=int, default=4096)
    ap.add_argument('--loop-rows', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    d = 4
    for N in [int(v) for v in a.sizes.split(',')]:
        M = N
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
        chain = a0 + 0.1 * rng.standard_normal((a.members, len(a0)))
        rows = chain[:min(a.loop_rows, len(chain))]
        out = dict(N=N, M=M, d=d, members=len(chain), samples=1)
        if not a.batched_only:
            def loop():
                for r in rows:
                    gp.sample(gp.active.array_to_dict(r))
            ms = median_ms(loop, max(2, a.reps // 2))
            out.update(loop_rows=len(rows), loop_us_per_row=1e3 * ms / len(rows), loop_rows_per_s=1e3 * len(rows) / ms)
        if not a.loop_only:
            ms = median_ms(lambda: gp.particles(chain), a.reps)
            out.update(particles_ms=ms, particles_rows_per_s=1e3 * len(chain) / ms, particles_us_per_row=1e3 * ms / len(chain))
            if 'loop_us_per_row' in out:
                out['speedup_per_row_vs_loop'] = out['loop_us_per_row'] / out['particles_us_per_row']
            if not a.batched_only:
                _, info = gp.sample_chain(chain, return_info=True)
                out.update(retry_share=float(np.mean(info['tries'] > 0)), fallback_share=float(np.mean(info['fallback'])),
                           max_tries=int(info['tries'].max()))
                dev = gp.device
                dev.prof_enable(2)
                dev.prof_reset()
                gp.particles(chain)
                pr = dev.prof_collect()
                dev.prof_enable(0)
                # event tags: gram = observation + prior Gram launches, potrf = observation factor + the robust posterior factor,
                # gemm_* = C -= V V^T
                ph = {k: round(v['ms'], 4) for k, v in pr.items() if v['count']}
                out.update(device_ms=ph, device_ms_tagged=round(sum(ph.values()), 4))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
