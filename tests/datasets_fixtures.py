"""Tiny raw datasets in the publishers' formats, synthesised from a seeded numpy generator (tests/test_datasets_*.py).
Each writer fills `<root>/raw/` and returns what it wrote, so a test can compare against the source of truth.
Only the Omniglot / COIL100 writers need Pillow (to encode PNGs); it is imported inside them."""
import gzip
import os
import pickle
import struct
import tarfile
import zipfile

import numpy as np

CIFAR10_NAMES = ['airplane', 'automobile', 'bird', 'cat', 'deer', 'dog', 'frog', 'horse', 'ship', 'truck']


def _dump(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump(obj, f, protocol=2)


def cifar10(root, seed=0, per_batch=32, test=7):
    """cifar-10-batches-py/{data_batch_1..5,test_batch,batches.meta}: `per_batch` images per train batch, `test` in the
    test batch.  -> {'train': (rows uint8 [5 * per_batch, 3072], labels), 'test': (...), 'classes': names}."""
    rng = np.random.default_rng(seed)
    top = os.path.join(root, 'raw', 'cifar-10-batches-py')
    rows, labels = {}, {}
    for name, n in [('data_batch_%d' % i, per_batch) for i in range(1, 6)] + [('test_batch', test)]:
        rows[name] = rng.integers(0, 256, (n, 3072), dtype=np.uint8)
        labels[name] = [int(v) for v in rng.integers(0, 10, n)]
        _dump(os.path.join(top, name), {'batch_label': name, 'labels': labels[name], 'data': rows[name],
                                        'filenames': ['%s_%d.png' % (name, i) for i in range(n)]})
    _dump(os.path.join(top, 'batches.meta'), {'label_names': CIFAR10_NAMES, 'num_vis': 3072, 'num_cases_per_batch': per_batch})
    train = ['data_batch_%d' % i for i in range(1, 6)]
    return {'train': (np.vstack([rows[n] for n in train]), np.array(sum((labels[n] for n in train), []), np.int64)),
            'test': (rows['test_batch'], np.array(labels['test_batch'], np.int64)), 'classes': CIFAR10_NAMES}


def cifar100(root, seed=1, train=9, test=4, fine=20):
    """cifar-100-python/{train,test,meta} with `fine` fine classes; coarse labels differ from the fine ones."""
    rng = np.random.default_rng(seed)
    top = os.path.join(root, 'raw', 'cifar-100-python')
    names = ['fine_%02d' % i for i in range(fine)]
    out = {'classes': names}
    for split, n in (('train', train), ('test', test)):
        rows = rng.integers(0, 256, (n, 3072), dtype=np.uint8)
        fine_labels = [int(v) for v in rng.integers(0, fine, n)]
        coarse_labels = [(v + 1) % fine for v in fine_labels]                     # never equal to the fine label
        _dump(os.path.join(top, split), {'data': rows, 'fine_labels': fine_labels, 'coarse_labels': coarse_labels,
                                         'filenames': ['%d.png' % i for i in range(n)]})
        out[split] = (rows, np.array(fine_labels, np.int64))
    _dump(os.path.join(top, 'meta'), {'fine_label_names': names, 'coarse_label_names': ['coarse_%d' % i for i in range(5)]})
    return out


def pack_tar_gz(src_root, dst_root, top, archive):
    """`src_root/raw/top/` -> `dst_root/raw/archive` (members named top/...), as the publisher's tarball is laid out."""
    os.makedirs(os.path.join(dst_root, 'raw'), exist_ok=True)
    with tarfile.open(os.path.join(dst_root, 'raw', archive), 'w:gz') as t:
        t.add(os.path.join(src_root, 'raw', top), arcname=top)


def pack_zip(src_root, dst_root, top, archive, reverse=True):
    """`src_root/raw/top/` -> `dst_root/raw/archive`; members in reverse order, so that sorting is the reader's work."""
    os.makedirs(os.path.join(dst_root, 'raw'), exist_ok=True)
    members = []
    for d, _, files in os.walk(os.path.join(src_root, 'raw', top)):
        members += [os.path.join(d, f) for f in files]
    with zipfile.ZipFile(os.path.join(dst_root, 'raw', archive), 'w') as z:
        z.writestr(top + '/', '')
        for p in sorted(members, reverse=reverse):
            z.write(p, os.path.relpath(p, os.path.join(src_root, 'raw')).replace(os.sep, '/'))


def idx_images(a):
    return struct.pack('>IIII', 2051, *a.shape) + a.tobytes()


def idx_labels(a):
    return struct.pack('>II', 2049, a.shape[0]) + a.astype(np.uint8).tobytes()


def mnist(root, seed=2, train=5, test=3, gz=False):
    """The four IDX files, plain or .gz.  -> {'train': (uint8 [n, 28, 28], labels), 'test': (...)}."""
    rng = np.random.default_rng(seed)
    raw = os.path.join(root, 'raw')
    os.makedirs(raw, exist_ok=True)
    out = {}
    for split, stem, n in (('train', 'train', train), ('test', 't10k', test)):
        img = rng.integers(0, 256, (n, 28, 28), dtype=np.uint8)
        lab = rng.integers(0, 10, n).astype(np.int64)
        for name, blob in (('%s-images-idx3-ubyte' % stem, idx_images(img)), ('%s-labels-idx1-ubyte' % stem, idx_labels(lab))):
            with (gzip.open(os.path.join(raw, name + '.gz'), 'wb') if gz else open(os.path.join(raw, name), 'wb')) as f:
                f.write(blob)
        out[split] = (img, lab)
    return out


OMNIGLOT_CLASSES = {'images_background': ['B_alpha/character01', 'B_alpha/character02', 'A_alpha/character01',
                                          'A_alpha/character02'],
                    'images_evaluation': ['AA_alpha/character01']}


def omniglot(root, seed=3, per_class=3):
    """images_background/{B_alpha,A_alpha}/character0{1,2}/ and images_evaluation/AA_alpha/character01/, `per_class`
    one-bit 105x105 PNGs each.  -> {path relative to raw/ with '/': 'Alphabet/characterNN'}."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = {}
    for tree, classes in OMNIGLOT_CLASSES.items():
        for c in classes:
            d = os.path.join(root, 'raw', tree, *c.split('/'))
            os.makedirs(d)
            for k in range(per_class):
                name = '%04d_%02d.png' % (rng.integers(0, 10000), k)
                Image.fromarray(rng.integers(0, 2, (105, 105)).astype(bool)).save(os.path.join(d, name))
                out['%s/%s/%s' % (tree, c, name)] = c
    return out


def coil100(root, seed=4, objects=('obj1', 'obj2', 'obj10'), views=(0, 5)):
    """coil-100/<obj>__<angle>.png, 128x128 RGB, plus a file that is no image.  -> {file name: object}."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = os.path.join(root, 'raw', 'coil-100')
    os.makedirs(d)
    out = {}
    for o in objects:
        for v in views:
            name = '%s__%d.png' % (o, v)
            Image.fromarray(rng.integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(os.path.join(d, name))
            out[name] = o
    with open(os.path.join(d, 'convertGroupppm2png.pl'), 'w') as f:
        f.write('not an image\n')
    return out

