"""g3_gp_append beside g3_gp_factor, and g3_gp_cross_append beside g3_gp_cross (profiles/append.md).

    python scripts/append_bench.py [--out FILE.json] [--reps 7] [--n0 8192 32768] [--m 1 128 1024] [--M 1024]

SE + noise, d = 3, fp64, inputs uniform on a box of side N^(1/3).  Host clock around calls that end in a device synchronise
(g3_gp_append and g3_gp_factor synchronise themselves; the cross entries are followed by g3_ctx_sync), one warm-up call of
every shape, then `reps` rounds that alternate the two sides; minimum and median per side.  Both append entries rewrite
everything from block row n0 on from the rows below it, so a repeated call does the same work on the same buffers."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clock(fn, sync=None):
    t0 = time.perf_counter()
    fn()
    if sync is not None:
        sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--n0', type=int, nargs='+', default=[8192, 32768])
    ap.add_argument('--m', type=int, nargs='+', default=[1, 128, 1024])
    ap.add_argument('--M', type=int, default=1024)
    args = ap.parse_args()
    import g3py_amd as g3
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    dev = g3.Device(0)
    d, t, P, M = 3, np.float64, _lib.G3_PAD, args.M
    rate = np.array([0.8, 1.0, 1.3])
    prog = compile_spec(('sum', ('SE', 1.3, rate, None), ('NOISE', 0.1)), d)
    cross = compile_spec(('SE', 1.3, rate, None), d)
    rows = []
    for N0 in args.n0:
        for m in args.m:
            N1 = N0 + m
            n0, Np1 = N0 // P * P, _lib.roundup(N1)
            r = Np1 - n0
            rng = np.random.default_rng(N1)
            side = N1 ** (1.0 / d)
            X = rng.uniform(0, side, (N1, d))
            y = np.sin(X.sum(axis=1) / np.sqrt(d)) + 0.1 * rng.standard_normal(N1)
            Xs = rng.uniform(0, side, (M, d))
            Xd, yd, Xsd = dev.upload(X), dev.upload(y), dev.upload(Xs)
            Mp = _lib.roundup(M)
            # side A: factor at N0, then append; side B: factor at N1 on buffers of its own
            KA, WA, aA = dev.alloc(Np1 + P, Np1, t), dev.alloc_inverses(Np1, t), dev.alloc(1, Np1, t)
            KB, WB, aB = dev.alloc(Np1 + P, Np1, t), dev.alloc_inverses(Np1, t), dev.alloc(1, Np1, t)
            VA, VB = dev.alloc(Mp, Np1, t), dev.alloc(Mp, Np1, t)
            mu, ss = dev.alloc(1, Mp, t), dev.alloc(1, Mp, t)
            st0 = dev.gp_factor(prog, Xd, N0, d, yd, KA, WA, aA)
            dev.gp_cross(cross, Xsd, M, Xd, N0, d, KA, WA, aA, VA, mu, ss)
            assert st0['tries'] == 0 and st0['info'] == 0
            app = lambda: dev.gp_append(prog, Xd, N0, N1, d, yd, KA, WA, aA)
            fac = lambda: dev.gp_factor(prog, Xd, N1, d, yd, KB, WB, aB)
            capp = lambda: dev.gp_cross_append(cross, Xsd, M, Xd, N0, N1, d, KA, WA, aA, VA, mu, ss)
            cfac = lambda: dev.gp_cross(cross, Xsd, M, Xd, N1, d, KB, WB, aB, VB, mu, ss)
            sa, sb = app(), fac()                      # warm-up, and the check that both sides computed the same thing
            assert sa['info'] == 0 and not sa['refused'] and sb['tries'] == 0
            assert abs(sa['logdet'] - sb['logdet']) <= 1e-10 * abs(sb['logdet']) and abs(sa['quad'] - sb['quad']) <= 1e-10 * sb['quad']
            capp(), cfac()
            dev.sync()
            T = dict(append=[], factor=[], cross_append=[], cross=[])
            for _ in range(args.reps):
                T['append'].append(clock(app))
                T['factor'].append(clock(fac))
                T['cross_append'].append(clock(capp, dev.sync))
                T['cross'].append(clock(cfac, dev.sync))
            flops_append = float(n0) * n0 * r + 2.0 * (r + P) * r * n0 + float(r) ** 3 / 3
            flops_factor = float(N1) ** 3 / 3
            row = dict(N0=N0, m=m, N1=N1, n0=n0, r=r, M=M, flop_ratio=flops_factor / flops_append,
                       **{k + '_min_ms': min(v) for k, v in T.items()}, **{k + '_med_ms': statistics.median(v) for k, v in T.items()})
            row['ratio'] = row['factor_min_ms'] / row['append_min_ms']
            row['cross_ratio'] = row['cross_min_ms'] / row['cross_append_min_ms']
            rows.append(row)
            print('N0 %6d m %5d r %5d: append %8.3f ms (median %8.3f)  factor at N1 %8.3f (%8.3f)  x%6.1f (flops x%6.1f) | '
                  'cross_append %7.3f (%7.3f)  cross %7.3f (%7.3f)  x%5.1f' % (
                      N0, m, r, row['append_min_ms'], row['append_med_ms'], row['factor_min_ms'], row['factor_med_ms'], row['ratio'],
                      row['flop_ratio'], row['cross_append_min_ms'], row['cross_append_med_ms'], row['cross_min_ms'],
                      row['cross_med_ms'], row['cross_ratio']), flush=True)
            # where an append's time goes: the library's event pairs around its regions, one call
            dev.prof_enable(True)
            dev.prof_reset()
            app()
            prof = dev.prof_collect()
            dev.prof_enable(False)
            row['append_regions_ms'] = {k: round(v['ms'], 4) for k, v in prof.items() if v['count']}
            print('    regions of one append, ms: %s' % row['append_regions_ms'], flush=True)
            for b in (Xd, yd, Xsd, KA, WA, aA, KB, WB, aB, VA, VB, mu, ss):
                b.free()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)
    dev.close()


if __name__ == '__main__':
    main()
