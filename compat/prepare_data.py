#!/usr/bin/env python3
"""Turn raw dataset files that are already on disk into what compat/data.py::fetch_dataset loads:

    python compat/prepare_data.py --data_name Omniglot [--root DIR]

reads DIR/raw/ (DIR: ./data/<data_name>, the reference's dataset root) and writes DIR/train.npz, DIR/test.npz and
DIR/meta.json (mcgen_amd/datasets.py::write_npz).  It is the reference's `process()` without its download step: nothing
is fetched, and when the raw files are not there the command lists what to place where and exits with status 1.
One line is printed per split: count, image shape, classes."""
import argparse
import os
import sys

import _path  # noqa: F401
import numpy as np

from mcgen_amd import datasets


def main(argv=None):
    ap = argparse.ArgumentParser(description='raw dataset files -> train.npz, test.npz, meta.json')
    ap.add_argument('--data_name', required=True, choices=datasets.DATA_NAMES)
    ap.add_argument('--root', default=None, help='dataset root holding raw/ (default ./data/<data_name>)')
    a = ap.parse_args(argv)
    root = datasets.default_root(a.data_name) if a.root is None else a.root
    try:
        meta = datasets.write_npz(a.data_name, root)
    except FileNotFoundError as e:
        print(e, file=sys.stderr)
        return 1
    for split in ('train', 'test'):
        with np.load(os.path.join(root, split + '.npz')) as z:
            print('{} {}: {} images {} uint8, {} classes -> {}'.format(
                a.data_name, split, meta['count'][split], list(z['img'].shape[1:]), meta['classes_size'],
                os.path.join(root, split + '.npz')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
