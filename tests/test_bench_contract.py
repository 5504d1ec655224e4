"""bench.py's one-line JSON contract: the fields the driver and the judge read, their types and their internal consistency --
on a committed line of the final tree (CPU) and on a fresh small run (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {'metric': str, 'value': float, 'unit': str, 'n_gpus': int, 'steps': int, 'warmup': int, 'ms_per_step': float,
            'higher_is_better': bool, 'scaling': str, 'dtype': str, 'data': str, 'config': dict}


def _check_line(j, n_gpus=1):
    for k, t in REQUIRED.items():
        assert k in j and isinstance(j[k], t), (k, type(j.get(k)))
    assert 'vs_baseline' in j and j['vs_baseline'] is None          # BASELINE.md holds no published number for this metric
    assert j['n_gpus'] == n_gpus and j['higher_is_better'] is True and j['data'] == 'synthetic'
    assert j['dtype'] in ('f64', 'f32') and 'workload' in j['config'] and 'model' not in j['config']
    # value = algorithmic flops of the step / measured time
    N, M = j['config']['N'], j['config']['M']
    sys.path.insert(0, ROOT)
    import bench
    flops = bench.step_flops(N, M, j['config'].get('draws', 0))
    if 'ms_per_step_median' in j:
        # round 4: value comes from the MEDIAN step, the mean stays beside it
        assert abs(j['value'] - flops / (j['ms_per_step_median'] * 1e-3) / 1e12) <= 1e-9 * j['value']
        assert abs(j['value_mean'] - flops / (j['ms_per_step'] * 1e-3) / 1e12) <= 1e-9 * j['value_mean']
    else:
        assert abs(j['value'] - flops / (j['ms_per_step'] * 1e-3) / 1e12) <= 1e-9 * j['value']
    r = j['roofline']
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] in ('GB/s', 'TFLOP/s')
    assert abs(r['frac'] - r['achieved'] / r['peak']) <= 1e-12 and 0 < r['frac'] < 1
    assert abs(r['achieved'] - r['avg_launch_flops'] / (r['avg_launch_ms'] * 1e-3) / 1e12) <= 1e-9 * r['achieved']
    assert r['traffic'] is None or r['traffic'] > 0
    if n_gpus == 1 and 'cpu_baseline' in j:
        c = j['cpu_baseline']
        assert c['kind'] in ('port', 'reference') and c['cores'] >= 1 and c['value'] > 0 and isinstance(c['sample'], str)


def test_committed_headline_line_keeps_the_contract():
    j = json.load(open(os.path.join(ROOT, 'profiles', 'r03_bench_final.json')))
    _check_line(j)
    assert j['config']['N'] == 32768 and j['dtype'] == 'f64' and 'cpu_baseline' in j and 'api_ms' in j
    assert j['logp_rel_err'] <= 1e-8                                # against the full-size oracle pin
    assert j['roofline']['traffic'] > j['roofline']['avg_launch_flops'] / 1e6   # bytes, not GB


def _r04_lines():
    import glob
    return sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r04_bench*.json')))


def test_round4_lines_median_value_roofline_everywhere_and_full_size_cpu_baseline():
    """(a) the headline line's cpu_baseline is a measured pass of the WHOLE N=32768 workload, (b) every
    committed line of the round carries `roofline`, (c) `value` comes from the median step with the mean beside it."""
    files = _r04_lines()
    names = [os.path.basename(f) for f in files]
    assert 'r04_bench.json' in names and 'r04_bench_c2.json' in names and 'r04_bench_c3.json' in names and 'r04_bench_c5.json' in names
    for f in files:
        j = json.load(open(f))
        if j.get('n_gpus', 1) != 1 or 'comm' in j:
            continue                                   # (lines of the multi-GPU driver are checked in test_gpu_distributed)
        _check_line(j)
        assert 'ms_per_step_median' in j and 'value_mean' in j, f
        assert 'roofline' in j and 0 < j['roofline']['frac'] < 1, f
    j = json.load(open(os.path.join(ROOT, 'profiles', 'r04_bench.json')))
    c = j['cpu_baseline']
    assert j['config']['N'] == 32768 and 'WHOLE workload' in c['sample'] and 'N=32768' in c['sample']
    assert c.get('extrapolation') is None and c['seconds'] > 1.0 and c['cores'] >= 1
    assert abs(c['logp'] - j['logp_ref']) <= 1e-8 * abs(j['logp_ref'])      # the CPU pass reproduces the pin, too


def test_step_flops_and_synthetic_inputs_are_what_survey_8d_states():
    sys.path.insert(0, ROOT)
    import bench
    N, M = 1000, 64
    assert bench.step_flops(N, M, 0) == pytest.approx(N ** 3 / 3.0 + N * N * (1 + M) + 2.0 * N * M, rel=1e-12)
    X, y, Xs = bench.synth(300, 3, 20, 1004)
    X2, y2, _ = bench.synth(300, 3, 20, 1004)
    assert np.array_equal(X, X2) and np.array_equal(y, y2) and X.shape == (300, 3) and Xs.shape == (20, 3)
    assert 0 <= X.min() and X.max() <= 300 ** (1 / 3) + 1e-12        # unit point density box
    assert bench.usable_cores() >= 1


def test_dump_outputs_keeps_float_types_and_samples_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: float32 stays float32, everything else is written as float64; an array over its share of the budget
    becomes a fixed sample of its entries -- the same one on every run"""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 1 << 16)
    big = np.arange(1 << 14, dtype=np.float64).reshape(128, 128)
    arrays = {'logp': np.array([-1.5]), 'mean': np.linspace(0, 1, 7, dtype=np.float32), 'count': np.arange(5), 'big': big}
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), arrays)
    total = 0
    for name in arrays:
        a, b = np.load(str(tmp_path / 'a' / (name + '.npy'))), np.load(str(tmp_path / 'b' / (name + '.npy')))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
        total += os.path.getsize(str(tmp_path / 'a' / (name + '.npy')))
    assert np.load(str(tmp_path / 'a' / 'mean.npy')).dtype == np.float32
    assert np.array_equal(np.load(str(tmp_path / 'a' / 'count.npy')), np.arange(5.0))
    s = np.load(str(tmp_path / 'a' / 'big.npy'))
    assert 0 < s.size < big.size and np.all(np.diff(s) > 0) and np.all(np.isin(s, big))   # sorted distinct entries of big
    assert total <= bench.DUMP_BUDGET_BYTES


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_last_step_computed(tmp_path):
    """a plain run carries the headline and nothing measured beside it; --dump-outputs holds the last timed step's
    results, which agree with the CPU oracle on the same synthetic inputs"""
    N, M = 4096, 256
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--points', str(N), '--queries', str(M), '--steps', '3',
                          '--warmup', '1', '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{'), lines[:5]
    j = json.loads(lines[0])
    for k, t in REQUIRED.items():
        assert k in j and isinstance(j[k], t), (k, type(j.get(k)))
    assert j['steps'] == 3 and j['warmup'] == 1 and j['dtype'] == 'f64' and j['ms_per_step'] > 0
    sys.path.insert(0, ROOT)
    import bench
    assert abs(j['value'] - bench.step_flops(N, M) / (j['ms_per_step_median'] * 1e-3) / 1e12) <= 1e-9 * j['value']
    for k in ('roofline', 'cpu_baseline', 'api_ms', 'logp_ref', 'phases_ms', 'cholesky_tflops', 'comm'):
        assert k not in j, k
    got = {n: np.load(str(tmp_path / (n + '.npy'))) for n in ('logp', 'logdet', 'quad', 'mean', 'ss', 'linv_delta')}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got['mean'].shape == (M,) and got['ss'].shape == (M,) and got['linv_delta'].shape == (N,)
    assert got['logp'][0] == j['logp']
    from oracle import g3_oracle as orc
    X, y, Xs = bench.synth(N, 4, M, 1004)
    lp, mean, var, _ = orc.cpu_hot_path(X, y, Xs)
    assert abs(got['logp'][0] - lp) <= 1e-9 * abs(lp)
    np.testing.assert_allclose(got['mean'], mean, rtol=0, atol=1e-8)
    np.testing.assert_allclose(np.maximum(1.0 - got['ss'], 0.0), var, rtol=0, atol=1e-8)
    assert abs(got['quad'][0] - got['linv_delta'].dot(got['linv_delta'])) <= 1e-10 * got['quad'][0]


@pytest.mark.gpu
def test_fresh_small_run_prints_one_contract_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--points', '4096', '--queries', '256', '--steps', '2',
                          '--warmup', '1', '--full', '--cpu-n', '1024', '--no-measure-traffic', '--no-api'], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{'), lines[:5]      # stdout carries the one line and nothing else
    j = json.loads(lines[0])
    _check_line(j)
    assert j['steps'] == 2 and j['warmup'] == 1 and j['config']['N'] == 4096 and 'cpu_baseline' in j


@pytest.mark.gpu
def test_one_rank_through_rccl_keeps_stdout_to_the_one_line():
    """G3_FORCE_DIST=1: the multi-GPU driver with one rank creates RCCL communicators, whose banner goes to the C stdout
    unless bench.py redirects it -- the line must still be alone, and carry the comm block"""
    env = dict(os.environ, G3_FORCE_DIST='1')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--points', '4096', '--queries', '256', '--steps', '1',
                          '--warmup', '1', '--full', '--cpu-n', '0', '--no-measure-traffic', '--no-api'], capture_output=True, text=True,
                         timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{'), lines[:5]
    j = json.loads(lines[0])
    assert j['comm']['driver'] == 'native' and j['comm']['per_rank'][0]['allgather']['calls_per_step'] > 0
    assert j['logp_ref'] is None if 'logp_ref' in j else True


@pytest.mark.gpu
def test_driver_downgrade_is_loud():
    """VERDICT r3 item 3d / ADVICE r3: when the native multi-GPU driver cannot be created the run says so in the line
    (`driver_fallback`) and FAILS, unless G3_DIST_ALLOW_FALLBACK=1 accepts the torch.distributed driver"""
    args = [sys.executable, os.path.join(ROOT, 'bench.py'), '--points', '2048', '--queries', '128', '--steps', '1', '--warmup', '1',
            '--full', '--cpu-n', '0', '--no-measure-traffic', '--no-api']
    env = dict(os.environ, G3_FORCE_DIST='1', G3_RCCL_PATH='/nonexistent/librccl.so')
    out = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith('{')]
    assert out.returncode != 0 and len(lines) == 1, (out.returncode, out.stderr[-1500:])
    j = json.loads(lines[0])
    assert 'driver_fallback' in j and 'librccl' in j['driver_fallback'] and j['comm']['driver'] == 'python'
    out = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(env, G3_DIST_ALLOW_FALLBACK='1'))
    assert out.returncode == 0, out.stderr[-1500:]
    assert 'driver_fallback' in json.loads([l for l in out.stdout.splitlines() if l.strip().startswith('{')][0])


@pytest.mark.gpu
def test_two_rank_rehearsal_runs_the_serial_pass_first_and_prints_both_in_one_line():
    """`bench.py --gpus N` (N > 1) runs the native driver twice in the same processes -- serial collective
    order first, then the overlapped default -- and prints ONE line with both passes; the headline is the faster pass that
    reproduced the pin.  Rehearsed with two ranks sharing the GPU over gloo (asynchronous callback transport)."""
    env = dict(os.environ, G3_DIST_BACKEND='gloo')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--points', '8192', '--queries', '1024', '--steps', '2',
                          '--warmup', '1', '--full', '--cpu-n', '0', '--no-measure-traffic', '--no-api', '--panel', '512'], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    _check_line(j, n_gpus=2)
    assert set(j['schedules']) == {'serial', 'overlapped'} and j['schedule'] in j['schedules']
    for k, v in j['schedules'].items():
        assert v['ms_per_step'] > 0 and v['pin_ok'] and v['logp_rel_err'] <= 1e-8, (k, v)
        assert len(v['comm']['per_rank']) == 2 and v['comm']['per_rank'][1]['allgather']['calls_per_step'] == 8192 // 512 - 1
    best = min(j['schedules'], key=lambda k: j['schedules'][k]['ms_per_step_median'])
    assert j['schedule'] == best and abs(j['ms_per_step_median'] - j['schedules'][best]['ms_per_step_median']) < 1e-9
    assert 'overlap_timeout' not in j and j['logp_rel_err'] <= 1e-8 and j['comm']['driver'] == 'native'


@pytest.mark.gpu
def test_overlapped_pass_that_never_returns_leaves_the_serial_line_and_a_failure():
    """... and if the overlapped pass runs into its limit the serial pass's line is printed with `overlap_timeout` and the run
    exits non-zero.  Forced here with a limit shorter than any pass."""
    env = dict(os.environ, G3_DIST_BACKEND='gloo', G3_BENCH_OVERLAP_LIMIT_S='0.001')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--points', '8192', '--queries', '1024', '--steps', '2',
                          '--warmup', '1', '--full', '--cpu-n', '0', '--no-measure-traffic', '--no-api', '--panel', '512'], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode != 0
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, (out.stdout[-2000:], out.stderr[-2000:])
    j = json.loads(lines[0])
    _check_line(j, n_gpus=2)
    assert j['overlap_timeout'] is True and j['schedule'] == 'serial' and list(j['schedules']) == ['serial']
    assert j['logp_rel_err'] <= 1e-8
