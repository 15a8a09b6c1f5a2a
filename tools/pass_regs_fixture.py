"""Writes tests/golden/pass_regs_parent.npz (GPU): the cases of tests/test_pass_regs_gpu.py run on the build the test is
to be compared with, i.e. the commit BEFORE a change to the pass step.  OSA_LIB_PATH selects that library (tools/ab_pass.sh
builds it from a revision):

    OSA_LIB_PATH=omnisafe_amd/lib/libomnisafe_amd_base.so python tools/pass_regs_fixture.py [destination.npz]

Prints every step's gradient norms next to the case's max_grad_norm, so that the clip / no-clip cases can be seen to be
what they are called."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_pass_regs_gpu as T  # noqa: E402


def main(argv):
    dst = argv[1] if len(argv) > 1 else os.path.join(ROOT, 'tests', 'golden', T.FIXTURE)
    blob = {}
    for name in sorted(T.CASES):
        _, res = T.run_case(name)
        assert all(np.isfinite(v).all() for v in res.values()), name
        print(f'{name:12s} max_grad_norm {T.CASES[name]["mgn"]:<6g} norms per step',
              np.array2string(res['stats'][:, 7:10], precision=4).replace('\n', ''))
        for key, val in T.stored(name, res).items():
            blob[f'{name}/{key}'] = val
    np.savez_compressed(dst, **blob)
    print(dst, os.path.getsize(dst), 'bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
