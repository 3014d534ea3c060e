"""Ingest CIFAR10 / CIFAR100 / MNIST / Omniglot / COIL100 from raw files already on disk (reference:
src/datasets/{cifar,mnist,omniglot,coil}.py and the transforms of src/data.py:19-55).

The reference's dataset classes fetch the publishers' archives on first use and decode / resize one PIL image per
`__getitem__`.  Here nothing is fetched: the user places the archives, or their extracted contents, under
`<root>/raw/` (the reference's `raw_folder`), and `ingest` turns them once, on the host, into what the device input
pipeline keeps in HBM (mcgen_amd/data.py): uint8 [N, 32, 32, C] images and int64 labels.  `write_npz` stores that as
`<root>/{train,test}.npz` + `<root>/meta.json`, the files `compat/data.py::fetch_dataset` loads.

Every input is read in place, extracted or as the shipped archive (tarfile / zipfile / gzip; nothing is unpacked to
disk), and both forms give identical arrays: members are addressed by their path relative to `raw/` with '/'
separators, and image lists are sorted by that path, so neither the file system's listing order nor the archive's member
order shows in the output.

Conventions restated from the reference:
  CIFAR10/100  rows of `data` -> [N, 3, 32, 32] -> NHWC, no resize (cifar.py:109-119); CIFAR100 uses the fine labels and
               the order of `fine_label_names` (cifar.py:105).
  MNIST        IDX files, 28x28 mode 'L' -> Resize((32, 32)) (mnist.py:163-180, data.py:22-24).
  Omniglot     class = 'Alphabet/characterNN' over images_background + images_evaluation, label = index in the sorted
               list of those strings; train = test = all images (omniglot.py:73-102); `.convert('L')`, then the resize.
  COIL100      class = filename.split('_')[0], label = index in the list sorted as strings; train = test = all images
               (coil.py:69-97); `.convert('RGB')`, then the resize.
`transforms.Resize((32, 32))` on a PIL image is `img.resize((32, 32), Image.BILINEAR)`; exactly that is called.
Pillow is imported only where an image is decoded or resized, so CIFAR ingests without it.
"""
from __future__ import annotations

import gzip
import io
import json
import os
import pickle
import struct
import tarfile
import zipfile
from typing import Dict, Iterable, List, Optional

import numpy as np

DATA_NAMES = ('MNIST', 'CIFAR10', 'CIFAR100', 'Omniglot', 'COIL100')
SIDE = 32
RESIZE = 'PIL BILINEAR 32x32'
_IMG_EXT = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif')      # datasets/utils.py:14

_CIFAR = {
    'CIFAR10': dict(top='cifar-10-batches-py', archive='cifar-10-python.tar.gz',
                    train=['data_batch_1', 'data_batch_2', 'data_batch_3', 'data_batch_4', 'data_batch_5'],
                    test=['test_batch'], meta='batches.meta', label_key='labels', names_key='label_names'),
    'CIFAR100': dict(top='cifar-100-python', archive='cifar-100-python.tar.gz', train=['train'], test=['test'],
                     meta='meta', label_key='fine_labels', names_key='fine_label_names'),
}
_MNIST = {'train': ('train-images-idx3-ubyte', 'train-labels-idx1-ubyte'),
          'test': ('t10k-images-idx3-ubyte', 't10k-labels-idx1-ubyte')}
_OMNIGLOT = ('images_background', 'images_evaluation')
_COIL = 'coil-100'


def default_root(data_name: str) -> str:
    return os.path.join('.', 'data', data_name)


def expected_raw(data_name: str) -> List[str]:
    """What `ingest` looks for under `<root>/raw/`, one line per input, for messages and documents."""
    if data_name in _CIFAR:
        c = _CIFAR[data_name]
        return ['{}/{{{}}}  or  {}'.format(c['top'], ','.join(c['train'] + c['test'] + [c['meta']]), c['archive'])]
    if data_name == 'MNIST':
        return ['{0}  or  {0}.gz'.format(n) for pair in _MNIST.values() for n in pair]
    if data_name == 'Omniglot':
        return ['{0}/<Alphabet>/<characterNN>/*.png  or  {0}.zip'.format(t) for t in _OMNIGLOT]
    if data_name == 'COIL100':
        return ['{0}/obj*__*.png  or  {0}.zip'.format(_COIL)]
    raise ValueError('Not valid dataset name')


def _missing(data_name: str, raw: str, what: Iterable[str]) -> FileNotFoundError:
    lines = ['{}: missing raw input {} under {}'.format(data_name, ', '.join(what), os.path.abspath(raw)),
             'Place there (nothing is downloaded):'] + ['  ' + e for e in expected_raw(data_name)]
    return FileNotFoundError('\n'.join(lines))


def _pil(data_name: str):
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError('{} is resized to 32x32 with Pillow (Image.resize, BILINEAR), which is not installed; only '
                          'CIFAR10 and CIFAR100 ingest without it'.format(data_name)) from e
    return Image


# ---- one raw input, extracted or archived -------------------------------------------------------------------------
class _Dir:
    """The extracted form: files under `raw/top/`, named by their path relative to `raw/` with '/' separators."""

    def __init__(self, raw: str, top: str):
        self.raw, self.top, self.where = raw, top, os.path.join(raw, top)

    def names(self) -> List[str]:
        out = []
        for d, _, files in os.walk(os.path.join(self.raw, self.top)):
            rel = os.path.relpath(d, self.raw).replace(os.sep, '/')
            out += ['{}/{}'.format(rel, f) for f in files]
        return sorted(out)

    def read(self, wanted: Iterable[str]) -> Dict[str, bytes]:
        out = {}
        for n in wanted:
            p = os.path.join(self.raw, *n.split('/'))
            if os.path.isfile(p):
                with open(p, 'rb') as f:
                    out[n] = f.read()
        return out


class _Zip:
    def __init__(self, path: str, top: str):
        self.where, self.top = path, top
        self.z = zipfile.ZipFile(path)
        self.files = {i.filename: i for i in self.z.infolist()
                      if not i.is_dir() and i.filename.startswith(top + '/')}

    def names(self) -> List[str]:
        return sorted(self.files)

    def read(self, wanted: Iterable[str]) -> Dict[str, bytes]:
        return {n: self.z.read(self.files[n]) for n in wanted if n in self.files}


class _Tar:
    """One sequential pass per `read`: seeking back in a .tar.gz decompresses it again from the start."""

    def __init__(self, path: str, top: str):
        self.where, self.top = path, top

    @staticmethod
    def _name(m) -> str:
        return m.name[2:] if m.name.startswith('./') else m.name

    def names(self) -> List[str]:
        with tarfile.open(self.where, 'r:*') as t:
            return sorted(self._name(m) for m in t if m.isfile() and self._name(m).startswith(self.top + '/'))

    def read(self, wanted: Iterable[str]) -> Dict[str, bytes]:
        wanted, out = set(wanted), {}
        with tarfile.open(self.where, 'r:*') as t:
            for m in t:
                if m.isfile() and self._name(m) in wanted:
                    out[self._name(m)] = t.extractfile(m).read()
        return out


def _source(raw: str, top: str, archive: str):
    """The extracted directory if it is there, else the archive, else None."""
    if os.path.isdir(os.path.join(raw, top)):
        return _Dir(raw, top)
    path = os.path.join(raw, archive)
    if os.path.isfile(path):
        return _Zip(path, top) if archive.endswith('.zip') else _Tar(path, top)
    return None


def _is_image(name: str) -> bool:
    return name.lower().endswith(_IMG_EXT)                               # datasets/utils.py:46-48


def _split(img: np.ndarray, label) -> Dict[str, np.ndarray]:
    return {'img': np.ascontiguousarray(img, dtype=np.uint8), 'label': np.asarray(label, dtype=np.int64)}


# ---- CIFAR ------------------------------------------------------------------------------------------------------------
def _cifar_batch(blob: bytes, where: str, label_key: str, classes: int):
    entry = pickle.loads(blob, encoding='latin1')
    if not isinstance(entry, dict) or 'data' not in entry or label_key not in entry:
        raise ValueError("{}: not a CIFAR batch (needs 'data' and '{}')".format(where, label_key))
    data, label = entry['data'], np.asarray(entry[label_key])
    if not isinstance(data, np.ndarray) or data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != 3 * SIDE * SIDE:
        raise ValueError("{}: 'data' is {} {}, expected uint8 [n, 3072]".format(
            where, getattr(data, 'dtype', type(data).__name__), list(getattr(data, 'shape', []))))
    if label.ndim != 1 or label.shape[0] != data.shape[0]:
        raise ValueError("{}: {} images but {} '{}'".format(where, data.shape[0], label.shape, label_key))
    if label.size and (label.min() < 0 or label.max() >= classes):
        raise ValueError("{}: '{}' outside [0, {})".format(where, label_key, classes))
    return data, label


def _ingest_cifar(data_name: str, raw: str):
    c = _CIFAR[data_name]
    src = _source(raw, c['top'], c['archive'])
    if src is None:
        raise _missing(data_name, raw, [c['top'] + '/', c['archive']])
    need = ['{}/{}'.format(c['top'], n) for n in c['train'] + c['test'] + [c['meta']]]
    blobs = src.read(need)
    if len(blobs) != len(need):
        raise _missing(data_name, raw, ['{} (in {})'.format(n, src.where) for n in need if n not in blobs])
    meta_name = need[-1]
    meta = pickle.loads(blobs[meta_name], encoding='latin1')
    if not isinstance(meta, dict) or c['names_key'] not in meta:
        raise ValueError("{} in {}: no '{}'".format(meta_name, src.where, c['names_key']))
    classes = [str(n) for n in meta[c['names_key']]]
    out = {'classes': classes}
    for split in ('train', 'test'):
        parts = [_cifar_batch(blobs['{}/{}'.format(c['top'], n)], '{}/{} in {}'.format(c['top'], n, src.where),
                              c['label_key'], len(classes)) for n in c[split]]
        img = np.vstack([p[0] for p in parts]).reshape(-1, 3, SIDE, SIDE).transpose(0, 2, 3, 1)
        out[split] = _split(img, np.concatenate([p[1] for p in parts]))
    return out


# ---- MNIST ------------------------------------------------------------------------------------------------------------
def _read_plain_or_gz(raw: str, name: str) -> Optional[bytes]:
    if os.path.isfile(os.path.join(raw, name)):
        with open(os.path.join(raw, name), 'rb') as f:
            return f.read()
    if os.path.isfile(os.path.join(raw, name + '.gz')):
        with gzip.open(os.path.join(raw, name + '.gz'), 'rb') as f:
            return f.read()
    return None


def parse_idx_images(blob: bytes, where: str) -> np.ndarray:
    """IDX3 (big-endian header: magic 2051, count, rows, cols; then count * rows * cols bytes) -> uint8 [n, rows, cols]."""
    if len(blob) < 16 or struct.unpack('>I', blob[:4])[0] != 2051:
        raise ValueError('{}: not an IDX image file (magic number is not 2051)'.format(where))
    n, rows, cols = struct.unpack('>III', blob[4:16])
    if len(blob) != 16 + n * rows * cols:
        raise ValueError('{}: header says {} images of {}x{} ({} bytes), the file holds {}'.format(
            where, n, rows, cols, 16 + n * rows * cols, len(blob)))
    return np.frombuffer(blob, dtype=np.uint8, offset=16).reshape(n, rows, cols)


def parse_idx_labels(blob: bytes, where: str) -> np.ndarray:
    """IDX1 (magic 2049, count; then count bytes) -> int64 [n]."""
    if len(blob) < 8 or struct.unpack('>I', blob[:4])[0] != 2049:
        raise ValueError('{}: not an IDX label file (magic number is not 2049)'.format(where))
    n = struct.unpack('>I', blob[4:8])[0]
    if len(blob) != 8 + n:
        raise ValueError('{}: header says {} labels ({} bytes), the file holds {}'.format(where, n, 8 + n, len(blob)))
    return np.frombuffer(blob, dtype=np.uint8, offset=8).astype(np.int64)


def _resize(pil_img, Image) -> np.ndarray:
    return np.asarray(pil_img.resize((SIDE, SIDE), Image.BILINEAR))     # transforms.Resize((32, 32)) on a PIL image


def _ingest_mnist(data_name: str, raw: str):
    blobs = {n: _read_plain_or_gz(raw, n) for pair in _MNIST.values() for n in pair}
    lost = [n for n, b in blobs.items() if b is None]
    if lost:
        raise _missing(data_name, raw, lost)
    Image = _pil(data_name)
    out = {'classes': [str(i) for i in range(10)]}
    for split, (img_name, label_name) in _MNIST.items():
        img = parse_idx_images(blobs[img_name], os.path.join(raw, img_name))
        label = parse_idx_labels(blobs[label_name], os.path.join(raw, label_name))
        if img.shape[0] != label.shape[0]:
            raise ValueError('{}: {} images in {} but {} labels in {}'.format(
                raw, img.shape[0], img_name, label.shape[0], label_name))
        if label.size and label.max() > 9:
            raise ValueError('{}: labels outside 0..9'.format(os.path.join(raw, label_name)))
        small = np.zeros((img.shape[0], SIDE, SIDE, 1), np.uint8)
        for i in range(img.shape[0]):
            small[i, :, :, 0] = _resize(Image.fromarray(img[i]), Image)     # uint8 [rows, cols] -> mode 'L' (mnist.py:33)
        out[split] = _split(small, label)
    return out


# ---- Omniglot / COIL100: image files, train = test = all of them ---------------------------------------------------------
def _decode_all(src_of: Dict[str, object], names: List[str], mode: str, Image) -> np.ndarray:
    out = np.zeros((len(names), SIDE, SIDE, len(mode)), np.uint8)
    for i, n in enumerate(names):
        blob = src_of[n].read([n])[n]
        try:
            with Image.open(io.BytesIO(blob)) as im:
                a = _resize(im.convert(mode), Image)
        except Exception as e:
            raise ValueError('{} in {}: not a readable image ({})'.format(n, src_of[n].where, e)) from e
        out[i] = a.reshape(SIDE, SIDE, len(mode))
    return out


def _ingest_omniglot(data_name: str, raw: str):
    srcs = {t: _source(raw, t, t + '.zip') for t in _OMNIGLOT}
    lost = [t + '/  or  ' + t + '.zip' for t, s in srcs.items() if s is None]
    if lost:
        raise _missing(data_name, raw, lost)
    Image = _pil(data_name)
    src_of = {}
    for s in srcs.values():
        src_of.update({n: s for n in s.names() if _is_image(n) and n.count('/') >= 3})
    names = sorted(src_of)
    if not names:
        raise _missing(data_name, raw, ['<Alphabet>/<characterNN>/*.png in ' + s.where for s in srcs.values()])
    cls = ['/'.join(n.split('/')[-3:-1]) for n in names]                  # omniglot.py:80
    classes = sorted(set(cls))
    index = {c: i for i, c in enumerate(classes)}
    both = _split(_decode_all(src_of, names, 'L', Image), [index[c] for c in cls])
    return {'train': both, 'test': both, 'classes': classes}


def _ingest_coil(data_name: str, raw: str):
    src = _source(raw, _COIL, _COIL + '.zip')
    if src is None:
        raise _missing(data_name, raw, [_COIL + '/', _COIL + '.zip'])
    Image = _pil(data_name)
    names = [n for n in src.names() if _is_image(n) and n.count('/') == 1]      # coil.py:70: the files of coil-100/ itself
    if not names:
        raise _missing(data_name, raw, ['obj*__*.png in ' + src.where])
    cls = [n.split('/')[-1].split('_')[0] for n in names]                 # coil.py:78
    classes = sorted(set(cls))                                             # as strings: obj1, obj10, obj100, obj11, ...
    index = {c: i for i, c in enumerate(classes)}
    both = _split(_decode_all({n: src for n in names}, names, 'RGB', Image), [index[c] for c in cls])
    return {'train': both, 'test': both, 'classes': classes}


_INGEST = {'CIFAR10': _ingest_cifar, 'CIFAR100': _ingest_cifar, 'MNIST': _ingest_mnist, 'Omniglot': _ingest_omniglot,
           'COIL100': _ingest_coil}


def ingest(data_name: str, root: Optional[str] = None) -> dict:
    """Read `<root>/raw/` (root: ./data/<data_name>) -> {'train': {'img': uint8 [N, 32, 32, C], 'label': int64 [N]},
    'test': {...}, 'classes': [names in label order]}.  FileNotFoundError (listing what to place where) when the raw
    files are not there, ValueError (naming the file) when one is malformed."""
    if data_name not in _INGEST:
        raise ValueError('Not valid dataset name')
    raw = os.path.join(default_root(data_name) if root is None else root, 'raw')
    if not os.path.isdir(raw):
        raise _missing(data_name, raw, ['the directory itself'])
    return _INGEST[data_name](data_name, raw)


def _replace_into(path: str, write) -> None:
    tmp = '{}.tmp{}'.format(path, os.getpid())
    try:
        with open(tmp, 'wb') as f:
            write(f)
        os.replace(tmp, path)                     # a reader never sees half a file
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def write_npz(data_name: str, root: Optional[str] = None) -> dict:
    """`ingest`, then `<root>/train.npz` and `<root>/test.npz` (arrays `img`, `label`) and `<root>/meta.json`;
    returns the meta dict."""
    root = default_root(data_name) if root is None else root
    got = ingest(data_name, root)
    for split in ('train', 'test'):
        _replace_into(os.path.join(root, split + '.npz'),
                      lambda f, s=got[split]: np.savez(f, img=s['img'], label=s['label']))
    meta = {'data_name': data_name, 'classes': got['classes'], 'classes_size': len(got['classes']),
            'count': {s: int(got[s]['img'].shape[0]) for s in ('train', 'test')},
            'resize': None if data_name in _CIFAR else RESIZE}
    _replace_into(os.path.join(root, 'meta.json'), lambda f: f.write(json.dumps(meta, indent=1).encode()))
    return meta
