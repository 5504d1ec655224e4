"""Gram-kernel throughput on MI355X (development aid): algorithmic GB/s = (N d s + bytes written) / time.
  python scripts/gram_bench.py [substring | ^prefix ...]     only the cases whose name contains a substring / starts with a prefix
Per case: 3 warm-up launches, then the MEDIAN (and min / max) of 15 launches timed one by one with device events."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import g3py_amd as g3
from g3py_amd import _lib
from g3py_amd.device import compile_spec
dev = g3.Device(0); st = torch.cuda.Stream(); torch.cuda.set_stream(st); dev.set_stream(st.cuda_stream)
cases = [('SE+noise d=4 N=32768 lower', ('sum', ('SE', 1.0, np.ones(4), None), ('NOISE', 0.1)), 32768, 4, True),
         ('SE+noise d=4 N=32768 full', ('sum', ('SE', 1.0, np.ones(4), None), ('NOISE', 0.1)), 32768, 4, False),
         ('MAT52+COS+noise d=8 N=16384 lower (config 3)', ('sum', ('sum', ('MAT52', 1.0, np.ones(8), None), ('COS', 0.5, np.full(8, 0.125), None)), ('NOISE', 0.1)), 16384, 8, True),
         ('MAT52+SIN+noise d=8 N=16384 lower', ('sum', ('sum', ('MAT52', 1.0, np.ones(8), None), ('SIN', 0.5, np.full(8, 0.125), np.full(8, 0.25), None)), ('NOISE', 0.1)), 16384, 8, True),
         ('MAT52+noise d=8 N=16384 lower (fast path)', ('sum', ('MAT52', 1.0, np.ones(8), None), ('NOISE', 0.1)), 16384, 8, True),
         ('RQ+noise d=4 N=16384 lower (fast path)', ('sum', ('RQ', 1.0, np.ones(4), 1.5, None), ('NOISE', 0.1)), 16384, 4, True),
         ('OU+noise d=4 N=16384 lower (fast path)', ('sum', ('OU', 1.0, np.ones(4), None), ('NOISE', 0.1)), 16384, 4, True),
         ('SE+noise d=16 N=16384 lower', ('sum', ('SE', 1.0, np.ones(16), None), ('NOISE', 0.1)), 16384, 16, True),
         ('SE+noise d=4 N=8192 lower (config 2)', ('sum', ('SE', 1.0, np.ones(4), None), ('NOISE', 0.1)), 8192, 4, True),
         # dot-product family (generated kernels; profiles/dot_gram.md).  '2*SE+0.1' is SE through the GENERATED kernel (the
         # compile-time table does not match a scaled / shifted kernel): it separates generated-vs-table from dot-vs-SE
         ('dot: LIN+noise d=4 N=32768 lower', ('sum', ('DOT', 1.0, np.ones(4), 0.5, 1, None), ('NOISE', 0.1)), 32768, 4, True),
         ('dot: LIN+SE+noise d=4 N=32768 lower', ('sum', ('sum', ('DOT', 1.0, np.ones(4), 0.5, 1, None), ('SE', 1.0, np.ones(4), None)), ('NOISE', 0.1)), 32768, 4, True),
         ('dot: NN+noise d=4 N=32768 lower', ('sum', ('NN', 1.0, np.ones(4), 0.5, None), ('NOISE', 0.1)), 32768, 4, True),
         ('dot: POL3+noise d=4 N=32768 lower', ('sum', ('DOT', 1.0, np.ones(4), 0.5, 3, None), ('NOISE', 0.1)), 32768, 4, True),
         ('dot: 2*SE+0.1+noise d=4 N=32768 lower (generated SE)', ('sum', ('shift', 0.1, ('scale', 2.0, ('SE', 1.0, np.ones(4), None))), ('NOISE', 0.1)), 32768, 4, True),
         ('dot: LIN+SE+noise d=8 N=32768 lower', ('sum', ('sum', ('DOT', 1.0, np.ones(8), 0.5, 1, None), ('SE', 1.0, np.ones(8), None)), ('NOISE', 0.1)), 32768, 8, True),
         ('SE+noise d=16 N=65536 lower fp32 (config 5 shape)', ('sum', ('SE', 1.0, np.ones(16), None), ('NOISE', 0.1)), 65536, 16, True, np.float32)]
only = sys.argv[1:]
for case in cases:
    name, spec, N, d, lower = case[:5]
    if only and not any(name.startswith(o[1:]) if o.startswith('^') else o in name for o in only):
        continue
    npdt = case[5] if len(case) > 5 else np.float64
    tdt = torch.float32 if npdt == np.float32 else torch.float64
    es = 4 if npdt == np.float32 else 8
    X = torch.rand((N, d), dtype=tdt, device='cuda') * N ** (1 / d)
    K = torch.empty((N, N), dtype=tdt, device='cuda')
    Xd, Kd = dev.wrap(X.data_ptr(), N, d, d, npdt), dev.wrap(K.data_ptr(), N, N, N, npdt)
    prog = compile_spec(spec, d)
    flags = _lib.G3_GRAM_SCRUB | (_lib.G3_GRAM_LOWER if lower else 0)
    for _ in range(3):
        dev.gram(prog, Xd, None, d, Kd, N, N, flags)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(15)]
    for e0, e1 in ev:
        e0.record()
        dev.gram(prog, Xd, None, d, Kd, N, N, flags)
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    ms = t[len(t) // 2]
    by = N * d * es + (N * (N + 1) / 2 if lower else N * N) * es
    del K
    print('%-56s %7.3f ms median (%.3f - %.3f)  %7.1f GB/s algorithmic' % (name, ms, t[0], t[-1], by / ms / 1e6))
