"""Builds libsurreal_mi.so (gfx950) in-tree from surreal_amd/csrc/*.hip.

Objects are compiled with hipcc for --offload-arch=gfx950 and linked against
the HIP runtime that ships inside torch (same SONAME libamdhip64.so.7), with a
RUNPATH to it, so a process that imports torch ends up with ONE HIP runtime
whichever library is loaded first.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(ROOT, 'build', 'obj')
LIB = os.path.join(HERE, 'libsurreal_mi.so')
HEADERS = ['smi_device.hpp', 'smi_internal.hpp', 'lstm_cell.hpp', 'pol_rows.hpp', 'mt19937.hpp',
           'gemm_args.hpp', 'dw_plan.hpp', 'smi_shapes.hpp', 'smi_launch.hpp', 'rnn_layout.hpp',
           'rnn_kernels.hpp', 'conv_plan.hpp', 'stem_plan.hpp']
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = 'gfx950'
CXXFLAGS = ['-O3', '-fPIC', '-std=c++17', f'--offload-arch={ARCH}', '-mcode-object-version=5',
            '-Wall', '-Wno-unused-function']
# Compilation units: (source, extra flags).  lstm_valu.hip, the VALU
# recurrence, is built with -fno-slp-vectorize (its fmaf chains stay scalar
# v_fmac_f32: the SLP vectorizer packs them into v_pk_fma_f32 + operand moves;
# measured at 128 segments, one MI355X: lstm_fwd 43.0 -> 40.9 us, lstm_bwd
# 34.5 -> 27.0 us per launch, learn 3.48 -> 3.29 ms; the flag on the MFMA forms
# of lstm_mfma.hip changed their rounding)
UNITS = [('ppo_gae.hip', []), ('ppo_epochs.hip', []), ('ops_kernels.hip', []),
         ('sampler_kernels.hip', []), ('per_kernels.hip', []),
         ('linear_kernels.hip', []), ('linear_dw.hip', []), ('ddpg_kernels.hip', []),
         ('dqn_kernels.hip', []),
         ('lstm_mfma.hip', []), ('lstm_valu.hip', ['-fno-slp-vectorize']), ('cnn_kernels.hip', []),
         ('conv_kernels.hip', []), ('stem.hip', []),
         ('head_kernels.hip', []), ('ppo_rnn_kernels.hip', []), ('ppo_rnn.hip', []),
         ('calib_kernels.hip', []), ('capi.hip', [])]


def torch_lib_dir():
    import torch
    return os.path.join(os.path.dirname(torch.__file__), 'lib')


def _mtime(p):
    return os.path.getmtime(p) if os.path.exists(p) else -1.0


# Developer variants: 'prof' adds the kernels' phase timers (-DSMI_PROF,
# tools/*_ticks.py, tools/lstm_breakdown.py, tools/fused_breakdown.py); 'fault'
# is the test-only fault injection (tests/negative_controls.py): the parity
# checks must FAIL on that build's deliberate departures.  The product library
# is variant None.
VARIANTS = {None: [], 'prof': ['-DSMI_PROF'], 'fault': ['-DSMI_FAULT_INJECTION']}


def lib_path(variant=None):
    return LIB if variant is None else LIB.replace('.so', f'_{variant}.so')


def build(verbose=False, force=False, variant=None):
    build_dir = BUILD if variant is None else f'{BUILD}_{variant}'
    lib = lib_path(variant)
    os.makedirs(build_dir, exist_ok=True)
    deps = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(ROOT, 'include', 'surreal_mi.h')]
    dep_t = max(_mtime(d) for d in deps)
    objs, cmds = [], []
    for src, extra in UNITS:
        sp = os.path.join(CSRC, src)
        op = os.path.join(build_dir, src.replace('.hip', '.o'))
        objs.append(op)
        if force or _mtime(op) < max(_mtime(sp), dep_t, _mtime(__file__)):
            cmds.append([HIPCC] + CXXFLAGS + extra + VARIANTS[variant] + ['-c', sp, '-o', op])
    # one hipcc per source, run side by side (each is single-threaded)
    from concurrent.futures import ThreadPoolExecutor
    jobs = max(1, min(len(cmds), int(os.environ.get('MAX_JOBS', os.cpu_count() or 1))))

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(run, cmds))
    if force or _mtime(lib) < max(_mtime(o) for o in objs):
        tl = torch_lib_dir()
        cmd = ['g++', '-shared', '-o', lib] + objs + [
            f'-L{tl}', '-l:libamdhip64.so', f'-Wl,-rpath,{tl}', '-Wl,--no-undefined', '-lstdc++']
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return lib


if __name__ == '__main__':
    var = next((a.split('=', 1)[1] for a in sys.argv if a.startswith('--variant=')), None)
    build(verbose=True, force='--force' in sys.argv, variant=var)
