"""Raw-file ingestion (mcgen_amd/datasets.py), its driver and loader hook (compat/prepare_data.py, compat/data.py) and the
image grids of compat/utils.py on the host.  Every raw file is synthesised in tmp_path (tests/datasets_fixtures.py); the
resize oracle is Pillow itself, called here; under test is everything around it: parsing, order, labels, archive forms."""
import json
import math
import os
import pickle
import struct
import subprocess
import sys

import numpy as np
import pytest

import datasets_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, 'compat')


def _nhwc(rows):
    return rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)


def _same(a, b):
    assert a['classes'] == b['classes']
    for split in ('train', 'test'):
        for k in ('img', 'label'):
            assert a[split][k].dtype == b[split][k].dtype and np.array_equal(a[split][k], b[split][k]), (split, k)


@pytest.fixture
def no_pillow(monkeypatch):
    """`import PIL` raises ImportError, as on a machine without Pillow."""
    for name in [m for m in sys.modules if m == 'PIL' or m.startswith('PIL.')]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, 'PIL', None)


# ---- CIFAR ------------------------------------------------------------------------------------------------------------
def test_cifar10_extracted_and_tarball(tmp_path, no_pillow):
    from mcgen_amd import datasets
    src = fx.cifar10(str(tmp_path / 'a'))
    got = datasets.ingest('CIFAR10', str(tmp_path / 'a'))
    assert got['classes'] == fx.CIFAR10_NAMES
    for split, n in (('train', 160), ('test', 7)):
        rows, labels = src[split]
        assert got[split]['img'].shape == (n, 32, 32, 3) and got[split]['img'].dtype == np.uint8
        assert got[split]['label'].shape == (n,) and got[split]['label'].dtype == np.int64
        assert np.array_equal(got[split]['img'], _nhwc(rows))                      # train: batch 1..5 in order
        assert np.array_equal(got[split]['label'], labels)
    assert got['train']['img'][33, 4, 5, 2] == src['train'][0][33, 2 * 1024 + 4 * 32 + 5]     # channel-major rows
    fx.pack_tar_gz(str(tmp_path / 'a'), str(tmp_path / 'b'), 'cifar-10-batches-py', 'cifar-10-python.tar.gz')
    assert os.listdir(tmp_path / 'b' / 'raw') == ['cifar-10-python.tar.gz']
    _same(got, datasets.ingest('CIFAR10', str(tmp_path / 'b')))
    assert os.listdir(tmp_path / 'b' / 'raw') == ['cifar-10-python.tar.gz']        # read in place, nothing unpacked
    assert 'PIL.Image' not in sys.modules


def test_cifar100_uses_fine_labels(tmp_path):
    from mcgen_amd import datasets
    src = fx.cifar100(str(tmp_path / 'a'))
    got = datasets.ingest('CIFAR100', str(tmp_path / 'a'))
    assert got['classes'] == src['classes'] and len(got['classes']) == 20
    for split in ('train', 'test'):
        assert np.array_equal(got[split]['img'], _nhwc(src[split][0]))
        assert np.array_equal(got[split]['label'], src[split][1])
    fx.pack_tar_gz(str(tmp_path / 'a'), str(tmp_path / 'b'), 'cifar-100-python', 'cifar-100-python.tar.gz')
    _same(got, datasets.ingest('CIFAR100', str(tmp_path / 'b')))


def test_cifar_malformed_batches(tmp_path):
    from mcgen_amd import datasets
    fx.cifar10(str(tmp_path))
    top = tmp_path / 'raw' / 'cifar-10-batches-py'
    good = (top / 'data_batch_3').read_bytes()
    entry = pickle.loads(good)
    for bad, word in ((dict(entry, data=entry['data'][:, :3000]), '3072'),                 # not [n, 3072]
                      (dict(entry, data=entry['data'].astype(np.int32)), 'uint8'),           # not uint8
                      (dict(entry, labels=entry['labels'][:-1]), 'labels'),                  # one label short
                      (dict(entry, labels=[10] + entry['labels'][1:]), 'labels')):           # a label without a class name
        fx._dump(str(top / 'data_batch_3'), bad)
        with pytest.raises(ValueError, match='data_batch_3') as e:
            datasets.ingest('CIFAR10', str(tmp_path))
        assert word in str(e.value)
    os.remove(top / 'data_batch_3')
    with pytest.raises(FileNotFoundError, match='data_batch_3'):
        datasets.ingest('CIFAR10', str(tmp_path))


# ---- MNIST ------------------------------------------------------------------------------------------------------------
def test_mnist_plain_and_gz(tmp_path):
    from PIL import Image
    from mcgen_amd import datasets
    src = fx.mnist(str(tmp_path / 'a'))
    assert fx.mnist(str(tmp_path / 'b'), gz=True)['train'][0].tobytes() == src['train'][0].tobytes()      # same seed, same content
    got = datasets.ingest('MNIST', str(tmp_path / 'a'))
    assert got['classes'] == [str(i) for i in range(10)]
    for split, n in (('train', 5), ('test', 3)):
        img, lab = src[split]
        assert got[split]['img'].shape == (n, 32, 32, 1) and got[split]['img'].dtype == np.uint8
        want = np.stack([np.asarray(Image.fromarray(a).resize((32, 32), Image.BILINEAR)) for a in img])
        assert np.array_equal(got[split]['img'][..., 0], want)
        assert np.array_equal(got[split]['label'], lab) and got[split]['label'].dtype == np.int64
    assert sorted(os.listdir(tmp_path / 'b' / 'raw')) == sorted(n + '.gz' for n in os.listdir(tmp_path / 'a' / 'raw'))
    _same(got, datasets.ingest('MNIST', str(tmp_path / 'b')))


def test_mnist_malformed(tmp_path):
    from mcgen_amd import datasets
    src = fx.mnist(str(tmp_path))
    raw = tmp_path / 'raw'
    images, labels = raw / 'train-images-idx3-ubyte', raw / 'train-labels-idx1-ubyte'
    good_i, good_l = images.read_bytes(), labels.read_bytes()
    images.write_bytes(struct.pack('>I', 2049) + good_i[4:])                       # wrong magic number
    with pytest.raises(ValueError, match='train-images-idx3-ubyte'):
        datasets.ingest('MNIST', str(tmp_path))
    images.write_bytes(good_i[:-100])                                              # truncated
    with pytest.raises(ValueError, match='train-images-idx3-ubyte'):
        datasets.ingest('MNIST', str(tmp_path))
    images.write_bytes(good_i + b'\0')                                             # one byte too many
    with pytest.raises(ValueError, match='train-images-idx3-ubyte'):
        datasets.ingest('MNIST', str(tmp_path))
    images.write_bytes(good_i)
    labels.write_bytes(struct.pack('>I', 2051) + good_l[4:])
    with pytest.raises(ValueError, match='train-labels-idx1-ubyte'):
        datasets.ingest('MNIST', str(tmp_path))
    labels.write_bytes(fx.idx_labels(src['train'][1][:4]))                         # 5 images, 4 labels
    with pytest.raises(ValueError, match='5 images'):
        datasets.ingest('MNIST', str(tmp_path))
    labels.write_bytes(good_l)
    assert datasets.ingest('MNIST', str(tmp_path))['train']['img'].shape[0] == 5


def test_resized_datasets_need_pillow(tmp_path, no_pillow):
    from mcgen_amd import datasets
    fx.mnist(str(tmp_path))
    with pytest.raises(ImportError, match='Pillow'):
        datasets.ingest('MNIST', str(tmp_path))


# ---- Omniglot ---------------------------------------------------------------------------------------------------------
def test_omniglot_trees_and_zips(tmp_path):
    from PIL import Image
    from mcgen_amd import datasets
    src = fx.omniglot(str(tmp_path / 'a'))
    got = datasets.ingest('Omniglot', str(tmp_path / 'a'))
    classes = sorted(['A_alpha/character01', 'A_alpha/character02', 'AA_alpha/character01', 'B_alpha/character01',
                      'B_alpha/character02'])
    assert got['classes'] == classes and classes[0] == 'AA_alpha/character01'       # from images_evaluation: both trees count
    assert got['train']['img'].shape == (15, 32, 32, 1)
    _same({'train': got['train'], 'test': got['train'], 'classes': classes}, got)   # train = test = all 15 images
    paths = sorted(src)                                                            # order: sorted paths relative to raw/
    assert np.array_equal(got['train']['label'], [classes.index(src[p]) for p in paths])
    differ = 0
    for i, p in enumerate(paths):
        with Image.open(tmp_path / 'a' / 'raw' / p) as im:
            assert im.mode == '1'
            want = np.asarray(im.convert('L').resize((32, 32), Image.BILINEAR))
            other = np.asarray(im.resize((32, 32), Image.BILINEAR).convert('L'))    # resizing the 1-bit image instead
        assert np.array_equal(got['train']['img'][i, :, :, 0], want), p
        differ += not np.array_equal(want, other)
    assert differ == 15                                                            # so the check above tells the two apart
    for tree in ('images_background', 'images_evaluation'):
        fx.pack_zip(str(tmp_path / 'a'), str(tmp_path / 'b'), tree, tree + '.zip')
    _same(got, datasets.ingest('Omniglot', str(tmp_path / 'b')))
    assert sorted(os.listdir(tmp_path / 'b' / 'raw')) == ['images_background.zip', 'images_evaluation.zip']
    os.remove(tmp_path / 'b' / 'raw' / 'images_evaluation.zip')                    # one tree alone is not the dataset
    with pytest.raises(FileNotFoundError, match='images_evaluation'):
        datasets.ingest('Omniglot', str(tmp_path / 'b'))


# ---- COIL100 ----------------------------------------------------------------------------------------------------------
def test_coil100_string_sorted_labels(tmp_path):
    from PIL import Image
    from mcgen_amd import datasets
    src = fx.coil100(str(tmp_path / 'a'))
    got = datasets.ingest('COIL100', str(tmp_path / 'a'))
    assert got['classes'] == ['obj1', 'obj10', 'obj2']                             # as strings, not numeric
    names = sorted(src)                                                            # the non-image file is not among them
    assert got['train']['img'].shape == (6, 32, 32, 3) and got['train']['img'].dtype == np.uint8
    assert np.array_equal(got['train']['label'], [{'obj1': 0, 'obj10': 1, 'obj2': 2}[src[n]] for n in names])
    for i, n in enumerate(names):
        with Image.open(tmp_path / 'a' / 'raw' / 'coil-100' / n) as im:
            want = np.asarray(im.convert('RGB').resize((32, 32), Image.BILINEAR))
        assert np.array_equal(got['train']['img'][i], want), n
    _same({'train': got['train'], 'test': got['train'], 'classes': got['classes']}, got)
    fx.pack_zip(str(tmp_path / 'a'), str(tmp_path / 'b'), 'coil-100', 'coil-100.zip')
    _same(got, datasets.ingest('COIL100', str(tmp_path / 'b')))


# ---- missing input, no network code ---------------------------------------------------------------------------------------
EXPECTED = {
    'CIFAR10': ['cifar-10-batches-py', 'data_batch_1', 'data_batch_2', 'data_batch_3', 'data_batch_4', 'data_batch_5',
                'test_batch', 'batches.meta', 'cifar-10-python.tar.gz'],
    'CIFAR100': ['cifar-100-python', 'train', 'test', 'meta', 'cifar-100-python.tar.gz'],
    'MNIST': ['train-images-idx3-ubyte', 'train-labels-idx1-ubyte', 't10k-images-idx3-ubyte', 't10k-labels-idx1-ubyte', '.gz'],
    'Omniglot': ['images_background', 'images_evaluation', 'images_background.zip', 'images_evaluation.zip'],
    'COIL100': ['coil-100', 'coil-100.zip'],
}


@pytest.mark.parametrize('data_name', sorted(EXPECTED))
@pytest.mark.parametrize('empty_raw', [False, True])
def test_missing_raw_lists_what_to_place_where(tmp_path, data_name, empty_raw):
    from mcgen_amd import datasets
    if empty_raw:
        os.makedirs(tmp_path / 'raw')
    with pytest.raises(FileNotFoundError) as e:
        datasets.ingest(data_name, str(tmp_path))
    for name in EXPECTED[data_name]:
        assert name in str(e.value), name
    assert str(tmp_path / 'raw') in str(e.value)
    with pytest.raises(ValueError):
        datasets.ingest('EMNIST', str(tmp_path))


def test_module_has_no_network_code():
    from mcgen_amd import datasets
    with open(datasets.__file__) as f:
        text = f.read()
    for word in ('urllib', 'requests', 'socket', 'http'):
        assert word not in text, word


# ---- write_npz, the driver, fetch_dataset ---------------------------------------------------------------------------------
@pytest.fixture
def compat_data(tmp_path, monkeypatch):
    """compat/data.py with ./ = tmp_path and the CPU as cfg['device']."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(COMPAT)
    import data as compat_data
    from mcgen_amd.config import cfg
    monkeypatch.setitem(cfg, 'device', 'cpu')
    monkeypatch.setitem(cfg, 'transform', None)
    return compat_data


def test_write_npz_then_fetch(tmp_path, compat_data, capsys):
    from mcgen_amd import datasets
    root = tmp_path / 'data' / 'COIL100'
    fx.coil100(str(root))
    got = datasets.ingest('COIL100')                                               # default root: ./data/<name>
    meta = datasets.write_npz('COIL100')
    assert meta == json.loads((root / 'meta.json').read_text())
    assert meta == {'data_name': 'COIL100', 'classes': ['obj1', 'obj10', 'obj2'], 'classes_size': 3,
                    'count': {'train': 6, 'test': 6}, 'resize': 'PIL BILINEAR 32x32'}
    assert sorted(os.listdir(root)) == ['meta.json', 'raw', 'test.npz', 'train.npz']
    ds = compat_data.fetch_dataset('COIL100')
    assert 'data ready (npz)\n' in capsys.readouterr().out
    for split in ('train', 'test'):
        assert not ds[split].synthetic and ds[split].classes_size == 3 and len(ds[split]) == 6
        assert np.array_equal(ds[split].img.numpy(), got[split]['img']) and ds[split].img.dtype.is_floating_point is False
        assert np.array_equal(ds[split].label.numpy(), got[split]['label'])
    os.remove(root / 'meta.json')                                                  # an npz alone: the table's class count, as before
    assert compat_data.fetch_dataset('COIL100', verbose=False)['train'].classes_size == 100


def test_fetch_ingests_raw_on_first_use(tmp_path, compat_data, capsys):
    root = tmp_path / 'data' / 'CIFAR10'
    src = fx.cifar10(str(root))
    ds = compat_data.fetch_dataset('CIFAR10')
    assert 'data ready (npz (ingested from raw))' in capsys.readouterr().out
    assert (root / 'train.npz').exists() and (root / 'test.npz').exists()
    assert json.loads((root / 'meta.json').read_text())['resize'] is None
    assert not ds['train'].synthetic and ds['train'].classes_size == 10
    assert np.array_equal(ds['train'].img.numpy(), _nhwc(src['train'][0])) and len(ds['test']) == 7
    assert np.array_equal(ds['train'].label.numpy(), src['train'][1])
    stamp = os.stat(root / 'train.npz').st_mtime_ns
    compat_data.fetch_dataset('CIFAR10')                                           # ingested once: now a plain load
    assert 'data ready (npz)\n' in capsys.readouterr().out and os.stat(root / 'train.npz').st_mtime_ns == stamp


def test_fetch_without_files_is_the_synthetic_stand_in(tmp_path, compat_data, capsys):
    ds = compat_data.fetch_dataset('Omniglot')
    assert capsys.readouterr().out == 'fetching data Omniglot...\ndata ready (synthetic stand-in (no ./data/Omniglot/*.npz))\n'
    assert ds['train'].synthetic and ds['train'].classes_size == 1623 and tuple(ds['train'].img.shape) == (2048, 32, 32, 1)
    assert os.listdir(tmp_path) == []


def _prepare(args, cwd):
    return subprocess.run([sys.executable, os.path.join(COMPAT, 'prepare_data.py')] + args, cwd=cwd, capture_output=True,
                          text=True, timeout=120, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))


def test_prepare_data_driver(tmp_path):
    fx.mnist(str(tmp_path / 'data' / 'MNIST'))
    r = _prepare(['--data_name', 'MNIST'], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and 'train: 5 images [32, 32, 1]' in lines[0] and 'test: 3 images [32, 32, 1]' in lines[1]
    assert all('10 classes' in line for line in lines)
    assert (tmp_path / 'data' / 'MNIST' / 'train.npz').exists()
    fx.coil100(str(tmp_path / 'elsewhere'))
    r = _prepare(['--data_name', 'COIL100', '--root', str(tmp_path / 'elsewhere')], tmp_path)
    assert r.returncode == 0 and '6 images [32, 32, 3]' in r.stdout and '3 classes' in r.stdout
    r = _prepare(['--data_name', 'CIFAR100'], tmp_path)                             # nothing there: says what to place where
    assert r.returncode == 1 and not (tmp_path / 'data' / 'CIFAR100' / 'train.npz').exists()
    assert 'cifar-100-python.tar.gz' in r.stderr and os.path.join('data', 'CIFAR100', 'raw') in r.stderr


# ---- make_grid / save_img ---------------------------------------------------------------------------------------------
def _grid_restated(x, nrow, padding, pad_value, rng):
    """torchvision's make_grid + save_image's byte conversion, cell by cell, in numpy fp32."""
    x = np.asarray(x, np.float32)
    if x.shape[1] == 1:
        x = np.concatenate([x, x, x], 1)
    if rng is not None:
        lo, hi = np.float32(rng[0]), np.float32(rng[1])
        x = (np.minimum(np.maximum(x, lo), hi) - lo) / (hi - lo + np.float32(1e-5))
    n, c, h, w = x.shape
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(n / xmaps))
    canvas = np.full((ymaps * (h + padding) + padding, xmaps * (w + padding) + padding, c), pad_value, np.float32)
    for row in range(ymaps):
        for col in range(xmaps):
            k = row * xmaps + col
            if k < n:
                top, left = padding + row * (h + padding), padding + col * (w + padding)
                canvas[top:top + h, left:left + w] = x[k].transpose(1, 2, 0)
    return np.floor(np.minimum(np.maximum(canvas * np.float32(255) + np.float32(0.5), 0), 255)).astype(np.uint8)


GRID_CASES = [  # n, c, nrow, padding, pad_value, range, scale of the input
    (7, 3, 3, 2, 0, (-1, 1), 1.3), (7, 3, 3, 0, 1, None, 1.0), (2, 3, 10, 2, 1, (0, 255), 300.0), (2, 1, 10, 0, 0, (-1, 1), 1.3),
    (7, 1, 3, 2, 1, None, 1.0), (7, 1, 3, 2, 0, (0, 255), 300.0), (2, 3, 10, 2, 0, None, 1.0), (12, 3, 4, 2, 1, (-1, 1), 1.3)]


@pytest.mark.parametrize('n,c,nrow,padding,pad_value,rng,scale', GRID_CASES)
def test_make_grid_and_save_img(tmp_path, monkeypatch, n, c, nrow, padding, pad_value, rng, scale):
    import torch
    from PIL import Image
    monkeypatch.syspath_prepend(COMPAT)
    import utils as compat_utils
    g = np.random.default_rng(n * 100 + c * 10 + padding)
    if rng is None:
        x = g.uniform(-0.2, 1.2, (n, c, 5, 6))                                     # past [0, 1]: the byte clamp is exercised
    else:
        x = g.uniform(-scale, scale, (n, c, 5, 6)) + (scale if rng[0] == 0 else 0) * 0.4        # past both ends of the range
    x = torch.from_numpy(x.astype(np.float32))
    want = _grid_restated(x.numpy(), nrow, padding, pad_value, rng)
    xmaps = min(nrow, n)
    assert want.shape == (math.ceil(n / xmaps) * (5 + padding) + padding, xmaps * (6 + padding) + padding, 3)
    got = compat_utils.make_grid(x, nrow, padding, pad_value, rng)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert 0 < (got == 0).sum() and 0 < (got == 255).sum() and np.unique(got).size > 20
    if n % xmaps and padding:                                                      # the ragged last row's empty cell
        assert (got[-(5 + padding):, -(6 + padding):] == (255 if pad_value else 0)).all()
    for ext in ('png', 'pdf'):
        compat_utils.save_img(x, str(tmp_path / 'vis' / f'grid.{ext}'), nrow=nrow, padding=padding, pad_value=pad_value, range=rng)
    with Image.open(tmp_path / 'vis' / 'grid.png') as im:
        assert im.mode == 'RGB' and np.array_equal(np.asarray(im), got)
    assert (tmp_path / 'vis' / 'grid.pdf').read_bytes().startswith(b'%PDF')
    assert np.array_equal(np.load(tmp_path / 'vis' / 'grid.npy'), x.numpy())       # the tensor itself, as before



_FRESH = '''
import sys
sys.path.insert(0, {compat!r})
import torch
from utils import save_img
save_img(torch.linspace(-1, 1, 2 * 3 * 4 * 4).view(2, 3, 4, 4), {path!r}, range=(-1, 1))
'''


def test_save_img_pdf_in_a_fresh_process(tmp_path):
    """A driver's first image may be a .pdf (save_format's default): Pillow's PDF writer needs the JPEG plugin registered,
    which a process that has opened or saved no other image has not done yet."""
    r = subprocess.run([sys.executable, '-c', _FRESH.format(compat=COMPAT, path=str(tmp_path / 'vis' / 'first.pdf'))],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / 'vis' / 'first.pdf').read_bytes().startswith(b'%PDF') and (tmp_path / 'vis' / 'first.npy').exists()
