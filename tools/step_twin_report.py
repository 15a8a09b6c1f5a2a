"""profiles/step_twin_error.md from the figures tests/test_step_oracle_gpu.py records on the GPU:

    OSA_STEP_TWIN_FIGURES=figures.json python -m pytest -m gpu tests/test_step_oracle_gpu.py
    python tools/step_twin_report.py figures.json > profiles/step_twin_error.md

A figure is (case, path, kind, network, what, measured, bound, single); kinds `<step>/grad` and `<step>/scalar` are ratios
error / max(e32, 2^-22), `<step>/adam` the parameter residual over its derived bound, `<step>/moments` ulps,
`<step>/state` chained moments / parameters over their tolerance.  `single` is the ratio against the SINGLE-order
float32 figure (rows as drawn) where `measured` is the ratio against the worst of four row orders, the tests' unit.
"""
import collections
import json
import sys


def main(path: str) -> None:
    fig = json.load(open(path))
    by = collections.defaultdict(float)   # (class, case, net, what, path) -> worst over the steps
    worst = collections.defaultdict(lambda: (0.0, None))
    bound = {}
    single = collections.defaultdict(lambda: (0.0, None))  # class, split into one-element quantities and tensors
    for case, p, kind, net, what, meas, bnd, sgl in fig:
        cls = kind.split('/')[1]
        if sgl is not None:
            key = cls if cls == 'scalar' else 'grad, one element' if what.endswith('4.bias') and net != 'actor' else 'grad'
            if sgl > single[key][0]:
                single[key] = (sgl, (case, p, kind, net, what))
        by[(cls, case, net, what, p)] = max(by[(cls, case, net, what, p)], meas)
        bound[cls] = bnd
        if meas > worst[cls][0]:
            worst[cls] = (meas, (case, p, kind, net, what))
    out = []
    w = out.append
    w('# The 64-row optimiser step against its float64 twin: measured error ratios (MI355X)\n')
    w('Written by `tools/step_twin_report.py` from one run of `tests/test_step_oracle_gpu.py` '
      f'({len(fig)} figures, {len({f[0] for f in fig})} cases, both paths).  A gradient or scalar entry is '
      '`error / max(e32, 2^-22)`: the relative L2 error of the kernel against `tests/step_twin.py` in float64, in units of '
      'what the float32 run of the same twin loses (`tests/golden/step_twin_f32_error.json`), worst over the '
      'minibatches of the case.  Columns `per-step / persistent`.\n')
    w('## Summary\n')
    w('| quantity | worst measured | where | bound in the test |')
    w('|---|---|---|---|')
    names = {'grad': 'gradient ratio (K_GRAD)', 'scalar': 'scalar ratio (K_SCALAR)',
             'adam': "parameter residual / (spacing(p) + 2e-6 abs(D))", 'moments': "moments [ulp]",
             'state': 'chained state / tolerance'}
    for cls in ('grad', 'scalar', 'adam', 'moments', 'state'):
        if cls in worst:
            m, (case, p, kind, net, what) = worst[cls]
            w(f'| {names[cls]} | {m:.2f} | {case}, {p}, {kind.split("/")[0]}, {net}, {what} | {bound[cls]:g} |')
    w('')
    w('K = the smallest power of two that is at least twice the worst measured ratio.\n')
    w('The unit `e32` of these ratios is the worst of four orders of the minibatch\'s rows (for a critic\'s one-element '
      'output bias: the larger of that and the typical size of the sum of its rows\' forward errors).  Against the '
      'float32 run with the rows as drawn alone -- one draw of the rounding error of every one-element quantity -- the '
      'worst ratios would be:\n')
    w('| quantity | worst ratio against the single-order figure | where |')
    w('|---|---|---|')
    for key in ('grad', 'grad, one element', 'scalar'):
        if key in single:
            m, (case, p, kind, net, what) = single[key]
            label = {'grad': 'gradient tensors of more than one element', 'grad, one element': "the critics' output bias",
                     'scalar': 'scalars'}[key]
            w(f'| {label} | {m:.2f} | {case}, {p}, {kind.split("/")[0]}, {net}, {what} |')
    w('')
    for cls, title in (('grad', 'Gradients, per case, network and reference tensor'),
                       ('scalar', 'Statistics and clip factor, per case and network')):
        w(f'## {title}\n')
        cases = []
        for key in by:
            if key[0] == cls and key[1] not in cases:
                cases.append(key[1])
        for net in ('actor', 'reward_critic', 'cost_critic'):
            cols = []
            for key in by:
                if key[0] == cls and key[2] == net and key[3] not in cols:
                    cols.append(key[3])
            if not cols:
                continue
            w(f'### {net}\n')
            w('| case | ' + ' | '.join(cols) + ' |')
            w('|---|' + '---|' * len(cols))
            for case in cases:
                cells = []
                for c in cols:
                    a, b = by.get((cls, case, net, c, 'per-step')), by.get((cls, case, net, c, 'persistent'))
                    cells.append('' if a is None and b is None else f'{a:.2f} / {b:.2f}')
                if any(cells):
                    w(f'| {case} | ' + ' | '.join(cells) + ' |')
            w('')
    w('## Adam, moments and chained state, per case\n')
    w('| case | network | quantity | per-step | persistent |')
    w('|---|---|---|---|---|')
    for key in sorted(k for k in by if k[0] in ('adam', 'moments') and k[4] == 'per-step'):
        cls, case, net, what, _ = key
        b = by.get((cls, case, net, what, 'persistent'))
        w(f'| {case} | {net} | {what} | {by[key]:.2f} | {b:.2f} |')
    sys.stdout.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main(sys.argv[1])
