#!/usr/bin/env python3
"""Driver counterpart of the reference's src/test_created.py:39-80: the Davies-Bouldin index of the created set.  Loads
output/npy/created_<model_tag>.npy (written by create.py --save_npy True), maps it back to (-1, 1), drops the samples that
hold a NaN together with their labels, and scores the rest with `Metric`'s DBI -- on the device when there is one
(mcgen_amd.metrics.davies_bouldin: only the score leaves HBM).  Prints the value and saves
output/result/dbi_created_<model_tag>.npy.  --raw True scores the training split itself instead
(output/result/dbi_created_<data_name>.npy)."""
import numpy as np
import torch

import _single  # noqa: F401  (sys.path)
import data as data_shim
from _single import cfg
from create import main
from data import fetch_dataset
from metrics import Metric
from utils import process_dataset, save


def _score(img, label, name):
    evaluation = Metric().evaluate(cfg['metric_name']['test'], None, {'img': img, 'label': label})
    print('Davies-Bouldin Index ({}): {}'.format(name, evaluation['DBI']))
    save(evaluation['DBI'], './output/result/dbi_created_{}.npy'.format(name), mode='numpy')
    return evaluation


def test(created):
    """test_created.py:66-80."""
    with torch.no_grad():
        created = torch.tensor(created / 255 * 2 - 1).to(cfg['device'])
        valid_mask = torch.sum(torch.isnan(created), dim=(1, 2, 3)) == 0
        label = torch.arange(cfg['classes_size'], device=created.device).repeat(cfg['generate_per_mode'])
        return _score(created[valid_mask], label[valid_mask], cfg['model_tag'])


def run_experiment(extra):
    """test_created.py:39-63."""
    seed = int(cfg['model_tag'].split('_')[0])
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    data_shim._SYNTHETIC['train'] = extra['synthetic_size']
    dataset = fetch_dataset(cfg['data_name'], cfg['subset'])
    process_dataset(dataset['train'])
    if cfg['raw']:
        from mcgen_amd.data import normalize_uint8
        train = dataset['train']
        with torch.no_grad():
            _score(normalize_uint8(train.img).contiguous(), train.label.long(), cfg['data_name'])
    else:
        test(np.load('./output/npy/created_{}.npy'.format(cfg['model_tag']), allow_pickle=True))


if __name__ == '__main__':
    main(run_experiment, {'metric_name': {'test': ['DBI']}})
