"""profiles/trust_twin_error.md from the figures tests/test_trust_oracle_gpu.py records on the GPU:

    OSA_TRUST_TWIN_FIGURES=figures.json python -m pytest -m gpu tests/test_trust_oracle_gpu.py
    python tools/trust_twin_report.py figures.json > profiles/trust_twin_error.md

A figure is (case, group, what, measured, bound, single).  Where the bound is K = 16, `measured` is error / unit with
unit = max(e32, 2^-22) of tests/golden/trust_twin_f32_error.json (for the scalars that carry them also the per-row and
log_std figures of tests/trust_twin.py) and `single` the same against the single-order float32 figures; the other
figures are element-wise residuals over their derived bounds, ulps, or the CG residual over the float32 twin's.
"""
import collections
import json
import sys

K = 16.0


def quantity(group: str, what: str) -> str:
    """The group of the summary a figure belongs to."""
    if group == 'fvp':
        return 'FVP: log_std block of osa_fvp_finish [ulp]' if 'ulp' in what else 'FVP tensors'
    if group == 'grad':
        return 'full-batch gradient: loss' if what.endswith('loss') else 'full-batch gradient tensors'
    if group == 'kl':
        return 'snapshot (mean rows)' if what.startswith('snapshot') else 'KL (PPOUpdater.kl)'
    if group == 'eval':
        return 'eval scalars: ' + what.split('/')[-1]
    if group == 'cg':
        return 'CG residual at k = 15 / float32 twin' if 'residual' in what else 'CG x_k, ' + what.replace('k', 'k = ')
    if group == 'cgdone':
        return 'CG with the done flag, x_k'
    if group == 'earlystop':
        return 'early stop: KL' if what.startswith('kl') else 'early stop: chained state / tolerance'
    return 'vector kernels: ' + what


def main(path: str) -> None:
    fig = json.load(open(path))
    worst = collections.OrderedDict()
    for case, group, what, meas, bound, single in fig:
        q = quantity(group, what)
        if q not in worst or meas > worst[q][0]:
            worst[q] = (meas, case, what, bound, single)
    out = []
    w = out.append
    w('# The trust-region and KL kernels against their float64 twin: measured error ratios (MI355X)\n')
    w(f'Written by `tools/trust_twin_report.py` from one run of `tests/test_trust_oracle_gpu.py` ({len(fig)} figures, '
      f'{len({f[0] for f in fig})} cases).  Where the bound is {K:g}, an entry is `error / unit`: the error of the kernel '
      'against `tests/trust_twin.py` in float64, in units of what the float32 run of the same twin loses '
      '(`tests/golden/trust_twin_f32_error.json`, floored at 2^-22).\n')
    w('## Summary\n')
    w('| quantity | worst measured | where | bound in the test | against the single-order figure |')
    w('|---|---|---|---|---|')
    for q, (meas, case, what, bound, single) in worst.items():
        w(f'| {q} | {meas:.2f} | {case}, {what} | {bound:g} | {"-" if single is None else f"{single:.2f}"} |')
    w('')
    top = max(m for m, _, _, b, _ in worst.values() if b == K)
    w(f'K = {K:g}: the smallest power of two that is at least twice the worst ratio measured against a unit ({top:.2f}).\n')
    by_case = collections.OrderedDict()
    for case, group, what, meas, bound, single in fig:
        by_case.setdefault((group, case), []).append((what, meas, bound))
    groups = collections.OrderedDict()
    for (group, case), rows in by_case.items():
        groups.setdefault(group, []).append((case, rows))
    for group, cases in groups.items():
        w(f'## {group}\n')
        if group == 'eval':  # 15 x 4 x 2 numbers per case: the worst over the fractions, per scalar and multiplier
            w('| case | quantity | worst ratio over j = 0 ... 14 | at j |')
            w('|---|---|---|---|')
            for case, rows in cases:
                best = collections.OrderedDict()
                for what, meas, _ in rows:
                    lam, j, q = what.split('/')
                    if (lam, q) not in best or meas > best[(lam, q)][0]:
                        best[(lam, q)] = (meas, j)
                for (lam, q), (meas, j) in best.items():
                    w(f'| {case} | {lam} {q} | {meas:.2f} | {j[1:]} |')
        else:
            w('| case | quantity | measured | bound |')
            w('|---|---|---|---|')
            for case, rows in cases:
                for what, meas, bound in rows:
                    w(f'| {case} | {what} | {meas:.2f} | {bound:g} |')
        w('')
    sys.stdout.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main(sys.argv[1])
