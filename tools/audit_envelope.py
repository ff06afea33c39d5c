"""Both tables of the envelope check (kgdet_amd/numerics.py) for a config on a synthetic batch (kgdet_amd/synthetic.py):
the weights every fp16-part convolution can be served from (EnvelopeGuard: max |w s|, counts beyond 255.875 / 511.75) and the
input activation of every dense convolution of one eval forward (numerics.audit: max |x|, counts beyond 65504 / 131008).

    python tools/audit_envelope.py CONFIG [CHECKPOINT]        CONFIG: a function of kgdet_amd/configs.py, e.g. kgdet_r50_fpn

The checkpoint is loaded under KGDET_ENVELOPE=off so that the tables show the weights as they are, whatever the policy would do.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    from kgdet_amd import build_detector, checkpoint, configs, numerics, synthetic
    cfg = getattr(configs, argv[1])()
    torch.manual_seed(0)
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    if len(argv) > 2:
        os.environ['KGDET_ENVELOPE'] = 'off'
        checkpoint.load_checkpoint(model, argv[2], map_location='cpu')
    model = model.cuda().eval()
    guard = numerics.EnvelopeGuard(model)
    rec = guard.table().run()
    print('weights: %d rows; limit %.3f, clamped beyond %.2f' % (len(guard.layers), numerics.WEIGHT_LIMIT, numerics.WEIGHT_CLAMP))
    print('%-60s %12s %9s %9s %9s' % ('layer', 'max |w s|', 'nonfinite', '> limit', '> clamp'))
    for l, r in zip(guard.layers, rec):
        flag = ' <--' if (r['nonfinite'] or r['over1']) else ''
        print('%-60s %12.6g %9d %9d %9d%s' % (l.name, r['max'], r['nonfinite'], r['over1'], r['over2'], flag))
    batch = synthetic.make_batch(1, 'cuda', seed=0)
    rows = numerics.audit(model, batch['img'])
    print('\nactivations of one eval forward: %d dense convolutions; fp32-class up to %g, 11 bits up to %g'
          % (len(rows), numerics.ACT_LIMIT, numerics.ACT_CLAMP))
    print('%-40s %-28s %12s %9s %9s %9s' % ('module#call', 'input, M, taps', 'max |x|', 'nonfinite', '> 65504', '> 131008'))
    for r in rows:
        flag = ' <--' if (r['nonfinite'] or r['over_limit']) else ''
        print('%-40s %-28s %12.6g %9d %9d %9d%s' % (r['name'], '%s %d %d' % r['shape'], r['max'], r['nonfinite'], r['over_limit'],
                                                    r['over_clamp'], flag))


if __name__ == '__main__':
    main(sys.argv)
