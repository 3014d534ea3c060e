#!/usr/bin/env python3
"""Driver counterpart of the reference's src/test_generated.py:39-79: Inception Score and FID of the generated set.  Loads
output/npy/generated_<model_tag>.npy (written by generate.py --save_npy True), maps it back to (-1, 1), drops the samples that
hold a NaN and scores the rest with `Metric`'s InceptionScore and FID (mcgen_amd.metrics: the reference's own classifier as the
feature network on COIL100 / Omniglot, its weights from ./metrics_tf/res/classifier/).  Prints both values and saves
output/result/is_generated_<model_tag>.npy and fid_generated_<model_tag>.npy.  --raw True scores the training split itself
instead (is_generated_<data_name>.npy, fid_generated_<data_name>.npy).  On the datasets the reference scores with torchvision's
pre-trained inception_v3 it fails with the message of mcgen_amd.metrics.feature_network."""
import numpy as np
import torch

import _single  # noqa: F401  (sys.path)
import data as data_shim
from _single import cfg
from create import main
from data import fetch_dataset
from metrics import Metric
from utils import process_dataset, save


def _score(img, name):
    """test_generated.py:53-59,73-78."""
    evaluation = Metric().evaluate(cfg['metric_name']['test'], None, {'img': img})
    is_result, fid_result = evaluation['InceptionScore'], evaluation['FID']
    print('Inception Score ({}): {}'.format(name, is_result))
    print('FID ({}): {}'.format(name, fid_result))
    save(is_result, './output/result/is_generated_{}.npy'.format(name), mode='numpy')
    save(fid_result, './output/result/fid_generated_{}.npy'.format(name), mode='numpy')
    return evaluation


def test(generated):
    """test_generated.py:66-79."""
    with torch.no_grad():
        generated = torch.tensor(generated / 255 * 2 - 1).to(cfg['device'])
        valid_mask = torch.sum(torch.isnan(generated), dim=(1, 2, 3)) == 0
        return _score(generated[valid_mask], cfg['model_tag'])


def run_experiment(extra):
    """test_generated.py:39-63."""
    from mcgen_amd.metrics import feature_network
    feature_network(cfg['data_name'], device=cfg['device'], subset=cfg.get('subset'))      # no feature network: say so before any work
    seed = int(cfg['model_tag'].split('_')[0])
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    data_shim._SYNTHETIC['train'] = extra['synthetic_size']
    dataset = fetch_dataset(cfg['data_name'], cfg['subset'])
    process_dataset(dataset['train'])
    if cfg['raw']:
        from mcgen_amd.data import normalize_uint8
        with torch.no_grad():
            _score(normalize_uint8(dataset['train'].img).contiguous(), cfg['data_name'])
    else:
        test(np.load('./output/npy/generated_{}.npy'.format(cfg['model_tag']), allow_pickle=True))


if __name__ == '__main__':
    main(run_experiment, {'metric_name': {'test': ['InceptionScore', 'FID']}})
