"""profiles/step_twin_error.md from the figures tests/test_step_oracle_gpu.py records on the GPU, and
profiles/step_forms_error.md from those of tests/test_step_forms_gpu.py (one file per run):

    OSA_STEP_TWIN_FIGURES=figures.json python -m pytest -m gpu tests/test_step_oracle_gpu.py
    python tools/step_twin_report.py figures.json > profiles/step_twin_error.md
    OSA_STEP_TWIN_FIGURES=forms.json python -m pytest -m gpu tests/test_step_forms_gpu.py
    python tools/step_twin_report.py forms.json > profiles/step_forms_error.md

profiles/general_twin_error.md likewise from tests/test_general_step_gpu.py (paths `general / apply`), and the
measuring stick of that file, on the CPU (the float32 twin against the float64 twin for step_twin.general_table()):

    python tools/step_twin_report.py --general-golden      # writes tests/golden/general_twin_f32_error.json
    OSA_STEP_TWIN_FIGURES=general.json python -m pytest -m gpu tests/test_general_step_gpu.py
    python tools/step_twin_report.py general.json > profiles/general_twin_error.md

and profiles/dp_twin_error.md from tests/test_dp_forms_gpu.py (paths dp-steps ... dp-split-spread, p2p; a gradient entry
there is the AVERAGED CLIPPED gradient, a scalar the mean over the ranks, the units those of step_twin.dp_f32_error):

    OSA_STEP_TWIN_FIGURES=dp.json python -m pytest -m gpu tests/test_dp_forms_gpu.py
    python tools/step_twin_report.py dp.json > profiles/dp_twin_error.md

The columns of the tables are the paths found in the figures, in their order of appearance (`per-step / persistent`
for the 64-row table; per-step, chunked, wide, split, split-spread, balanced, strided for the forms, where a case runs
on the forms of its family only and the other cells stay `-`).

A figure is (case, path, kind, network, what, measured, bound, single); kinds `<step>/grad` and `<step>/scalar` are ratios
error / max(e32, 2^-22), `<step>/adam` the parameter residual over its derived bound, `<step>/moments` ulps,
`<step>/state` chained moments / parameters over their tolerance.  `single` is the ratio against the SINGLE-order
float32 figure (rows as drawn) where `measured` is the ratio against the worst of four row orders, the tests' unit.
"""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def general_golden() -> None:
    """tests/golden/general_twin_f32_error.json: step_twin.f32_error of every case of general_table(), one thread."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import step_twin as T
    import torch

    torch.set_num_threads(1)
    table = {}
    for name, e in T.general_table().items():
        table[name] = T.f32_error(T.make_case(**e['kw']))
        print(name, file=sys.stderr)
    blob = T.pack_general_error(table)
    dst = os.path.join(ROOT, 'tests', 'golden', 'general_twin_f32_error.json')
    with open(dst, 'w') as fh:
        fh.write('{"cases": {\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in blob['cases'].items()) + '}}\n')
    print(dst, os.path.getsize(dst), 'bytes', file=sys.stderr)


def main(path: str) -> None:
    fig = json.load(open(path))
    paths = []
    for f in fig:
        if f[1] not in paths:
            paths.append(f[1])
    narrow = paths == ['per-step', 'persistent']
    general = 'general' in paths
    dp = any(q.startswith('dp-') for q in paths)  # tests/test_dp_forms_gpu.py (its last column, p2p: cases and units of the 64-row table)
    per_path = collections.defaultdict(lambda: (0.0, None))  # (class, path) -> worst
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
        bound.setdefault(cls, bnd)
        if meas > worst[cls][0]:
            worst[cls] = (meas, (case, p, kind, net, what))
            bound[cls] = bnd  # (the bound of the worst figure: v' after a zero-moment step has 4 ulp, the seeded recurrences 2)
        if meas > per_path[(cls, p)][0]:
            per_path[(cls, p)] = (meas, (case, p, kind, net, what))
    out = []
    w = out.append
    cols_txt = ' / '.join(paths)
    w('# The 64-row optimiser step against its float64 twin: measured error ratios (MI355X)\n' if narrow else
      '# The optimiser step of general networks against the float64 twin: measured error ratios (MI355X)\n' if general else
      '# The data-parallel forms of the optimiser step against the float64 twin: measured error ratios (MI355X)\n' if dp else
      '# The chunked, wide, split and large-batch steps against the float64 twin: measured error ratios (MI355X)\n')
    w('Written by `tools/step_twin_report.py` from one run of '
      + ('`tests/test_step_oracle_gpu.py` ' if narrow else '`tests/test_general_step_gpu.py` ' if general
         else '`tests/test_dp_forms_gpu.py` ' if dp else '`tests/test_step_forms_gpu.py` ') +
      f'({len(fig)} figures, {len({f[0] for f in fig})} cases, '
      + ('both paths' if narrow else f'{len({(f[0], f[1]) for f in fig})} (case, form) pairs') + ').  A gradient or scalar entry is '
      '`error / max(e32, 2^-22)`: the relative L2 error of the kernel against `tests/step_twin.py` in float64, in units of '
      'what the float32 run of the same twin loses (`tests/golden/'
      + ('general_twin' if general else 'dp_twin' if dp else 'step_twin') + '_f32_error.json`), worst over the '
      f'minibatches of the case.  Columns `{cols_txt}`' + ('' if narrow else ' (`-`: the case does not run on that form)') + '.\n')
    if dp and 'p2p' in paths:
        w('The last column, `p2p`, is the peer-exchange pass at a world of one on three cases of the 64-row table: single-rank '
          'twin, units from `tests/golden/step_twin_f32_error.json`.\n')
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
    w('K = the smallest power of two that is at least twice the worst measured ratio.\n' if narrow else
      'The bounds are those of the 64-row table (`tests/test_step_oracle_gpu.py`; a clipped gradient of mode 1 adds the '
      'clip factor\'s bound to its tensor\'s and is listed rescaled to K_GRAD); nothing was fitted to this path.\n' if general else
      'The bounds are those of the 64-row table (`tests/test_step_oracle_gpu.py`); nothing was fitted to these forms.  '
      + ('Every quantity stayed inside its bound in the units of the float32 twin of the data-parallel step (the '
         'averaged clipped gradient, the rank-mean scalars): no unit was re-derived for these forms.\n'
         if dp and all(f[5] <= f[6] for f in fig) else
         'Every quantity stayed inside its bound in the units of the float32 twin (the sums over up to 6000 rows and '
         'the slab sums of the large-batch forms included): no unit was re-derived for these forms.\n'
         if all(f[5] <= f[6] for f in fig) else
         'NOT every quantity stayed inside its bound: see the rows above.\n'))
    if not narrow:
        w('## Worst ratio per form\n')
        w('| form | ' + ' | '.join(names[c] for c in ('grad', 'scalar', 'adam', 'moments', 'state')) + ' |')
        w('|---|' + '---|' * 5)
        for p in paths:
            cells = []
            for cls in ('grad', 'scalar', 'adam', 'moments', 'state'):
                m, where = per_path[(cls, p)]
                cells.append('-' if where is None else f'{m:.2f} ({where[0]}, {where[3]}, {where[4]})')
            w(f'| {p} | ' + ' | '.join(cells) + ' |')
        w('')
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
                    vals = [by.get((cls, case, net, c, p)) for p in paths]
                    cells.append('' if all(v is None for v in vals)
                                 else ' / '.join('-' if v is None else f'{v:.2f}' for v in vals))
                if any(cells):
                    w(f'| {case} | ' + ' | '.join(cells) + ' |')
            w('')
    w('## Adam, moments and chained state, per case\n')
    w('| case | network | quantity | ' + ' | '.join(paths) + ' |')
    w('|---|---|---|' + '---|' * len(paths))
    for key in sorted({k[:4] for k in by if k[0] in ('adam', 'moments')}):
        cls, case, net, what = key
        vals = [by.get(key + (p,)) for p in paths]
        w(f'| {case} | {net} | {what} | ' + ' | '.join('-' if v is None else f'{v:.2f}' for v in vals) + ' |')
    sys.stdout.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    if sys.argv[1] == '--general-golden':
        general_golden()
    else:
        main(sys.argv[1])
