"""Generate tests/golden/ref_configs_golden.txt from the reference's config files (needs a reference checkout):

    python tests/golden/make_config_golden.py <reference checkout>/configs

Each config is evaluated by kgdet_amd.registry.Config.fromfile, and the objects the detector is built from --
``model``, ``train_cfg`` and ``test_cfg`` -- are written as one Python literal (``ast.literal_eval`` reads it back
with tuples, floats and key order intact), keyed by the config's name.  The file holds only data: no code of the
configs (data pipelines, schedules, paths) is kept."""
import os
import pprint
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from kgdet_amd.registry import Config  # noqa: E402

NAMES = ('kgdet_moment_r50_fpn_1x-demo', 'kgdet_moment_r50_fpn_1x-deepfashion2',
         'reppoints_moment_serial_r50_fpn_1x-deepfashion2', 'reppoints_moment_parallel_r50_fpn_1x-deepfashion2')
KEYS = ('model', 'train_cfg', 'test_cfg')


def main(cfg_dir):
    out = {}
    for name in NAMES:
        cfg = Config.fromfile(os.path.join(cfg_dir, name + '.py'))
        out[name] = {k: cfg[k] for k in KEYS}
    path = os.path.join(HERE, 'ref_configs_golden.txt')
    with open(path, 'w') as f:
        f.write(pprint.pformat(out, width=120, sort_dicts=False) + '\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
