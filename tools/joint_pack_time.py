"""Host time of the joint stages' packing, without a device.
Usage: python tools/joint_pack_time.py [--calls 200] [--label TEXT] [--out FILE] [--device]

The engine of tests/joint_pack_capture.py (CPU tensors, a native library that
answers 0) runs three calls over and over; what is timed is everything
Engine.run_joint* does on the host around the native call: checks, rows,
uploads (here: copies), the args struct.
  continuous  run_joint, 16 dimensions, 40 trials, 2 ids, 64 candidates
  quantised   run_joint_quant, 2 continuous + 1 discrete + 2 quantised (V = 50, 7)
  segmented   run_joint_segments over workload (c) of
              tools/joint_branch_mixed_time.py at its --small sizes
--device: the same three calls on cuda:0 through the real library (TPE_HIP_LIB
picks an A/B build), so that the native driver's checks, fills and launches are
in the time too; a call ends when its records are on the host.
One JSON line (per workload the median, the quartiles, min and max in ms) goes
to stdout and, with --out, is appended there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    ap.add_argument('--device', action='store_true')
    args = ap.parse_args()
    from tests import joint_pack_capture as K
    from tools.joint_branch_mixed_time import SEED, make_group
    cont, quant = K.cont_group(16), K.quant_group(*K.QUANT_CASES['2_1_50_7'])
    models = [make_group(200, SEED + s) for s in range(8)]
    words = [0xFFFFFFFE - 5 * s for s in range(8)]
    prob_id, prob_seg = np.arange(200, 264, dtype=np.int64), np.arange(64) % 8
    work = dict(continuous=lambda e: e.run_joint(*cont, K.IDS, K.C, K.SEED),
                quantised=lambda e: e.run_joint_quant(*quant, K.IDS, K.C, K.SEED),
                segmented=lambda e: e.run_joint_segments(models, words, prob_seg, prob_id, 4096, SEED))
    line = dict(tool='joint_pack_time', label=args.label, calls=args.calls, device=args.device, ms={})
    if args.device:
        import torch
        from hyperopt_amd.engine import get_engine
        dev_eng = get_engine(torch.device('cuda', 0))
    for name, fn in work.items():
        eng = dev_eng if args.device else K.stub_engine()[0]
        clear = (lambda: None) if args.device else eng.lib.calls.clear
        for _ in range(10):
            fn(eng)
        clear()
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn(eng)
            ms.append((time.perf_counter() - t0) * 1e3)
            clear()
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        line['ms'][name] = dict(median=float(med), q1=float(q1), q3=float(q3), min=float(min(ms)), max=float(max(ms)))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
