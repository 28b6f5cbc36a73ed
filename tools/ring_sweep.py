"""The lean f64 kernels' first-hit ring (csrc/rt_launch.h HIT_RING_QN, HIT_RING_FILL_AT and their _COMPACT twins) swept over builds of the
lean unit (tools/mkab_lean.sh qnQ_fF "-DRT_HIT_RING_QN=Q -DRT_HIT_RING_FILL_AT=F" for the wide form, cqQ_fF "-DRT_HIT_RING_QN_COMPACT=Q
-DRT_HIT_RING_FILL_AT_COMPACT=F" for the compact one, which is what the Cornell box runs; add -DRT_HIT_RING_ANY_SIZE for a size that gives
up the fifth workgroup per CU — its counters still count; --wide: RT_NO_ONB_TABLE for the whole run, so that the Cornell box runs the
wide form): one 800 x 800 x spp frame of C2's scene and view per library,
and per library the loop counters, which depend on the per-wave logic only (not on occupancy or clocks): wave iterations per 64 samples
and lanes live at a search; beside them the LDS of a workgroup and what the runtime answers for resident workgroups per CU.
usage: python tools/ring_sweep.py [--spp 128] name=lib.so ..."""
import argparse, ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: F401  (one HIP runtime in the process)
from raytracinginrust_amd import _lib, scenes
ap = argparse.ArgumentParser(); ap.add_argument('--spp', type=int, default=128); ap.add_argument('--size', type=int, default=800); ap.add_argument('libs', nargs='+')
ap.add_argument('--wide', action='store_true')
a = ap.parse_args()
if a.wide: os.environ['RT_NO_ONB_TABLE'] = '1'      # (read when a scene is flattened: no valid entry, the wide ring)
W = H = a.size
ref = None
print(f'# Cornell box {W} x {H} x {a.spp}, max_depth 50, f64')
print(f'# {"build":16s} {"iterations / 64 samples":>24s} {"lanes live at a search":>24s} {"LDS B / workgroup":>18s} {"workgroups / CU":>16s} {"kernel ms":>10s}  frame')
for spec in a.libs:
    name, path = spec.split('=', 1)
    be = _lib.load_path(os.path.abspath(path), allow_missing=True); b, cam, bg = scenes.cornell_box(be)
    out = np.zeros((H, W, 3))
    assert be.lib.rt_render(b.h, C.byref(cam), (C.c_double * 3)(*bg), W, H, a.spp, 50, 0x5EED, 0, out.ctypes.data) == 0
    ms = C.c_float(); be.lib.rt_last_kernel_ms(b.h, C.byref(ms))
    st = (C.c_ulonglong * 3)(); be.lib.rt_last_stats(b.h, st)
    info = (C.c_uint32 * 6)(); be.lib.rt_last_launch_info(b.h, info)
    if ref is None: ref = out
    d = float(np.nanmax(np.abs(out - ref)))
    print(f'  {name:16s} {st[1] * 64.0 / (W * H * a.spp):24.4f} {st[2] / float(st[1]):24.3f} {info[2]:18d} {info[5]:16d} {ms.value:10.3f}  '
          f'nonfinite {st[0]}, max |diff| vs {a.libs[0].split("=")[0]} {d:.2e}', flush=True)
