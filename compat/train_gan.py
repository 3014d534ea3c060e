#!/usr/bin/env python3
"""Driver counterpart of the reference's src/train_gan.py for the MI355X path: same CLI flags
(train_gan.py:18-28: --data_name --model_name --control_name --world_size --num_epochs --init_seed --resume_mode
...), same experiment structure (runExperiment -> train / test per epoch -> checkpoint in the reference's dict
layout, train_gan.py:58-122), same loop body (train_gan.py:139-176).

What differs, and why:
  * the dataset is synthetic and lives on the device (this image ships no datasets and has no network; the
    reference's own `datasets` package needs torchvision): uint8 images + labels, normalised to (-1, 1) and batched
    on the GPU by `mcgen_amd.data.DeviceLoader` (data.py:19-55,65-82: ToTensor + Normalize(0.5, 0.5), shuffle);
  * `--engine fused` (default) runs the loop body as `GraphedGANTrainer` (fused Adam, HIP-graph replay);
    `--engine autograd` runs the reference's own Python loop on the nn.Module surface with the torch.optim class; either
    way the optimizer is cfg['optimizer_name'] ('Adam' unless --optimizer_name / --momentum, compat/_flags.py, say otherwise);
  * --world_size > 1 means one process per GPU under torch.distributed.run (RCCL), not nn.DataParallel;
  * test() generates `generate_per_mode` images per class (train_gan.py:197-207).  On COIL100 / Omniglot, with the trained
    feature classifier at ./metrics_tf/res/classifier/ (where the reference keeps it; compat/train_classifier.py writes it),
    it logs 'test/InceptionScore' and 'test/FID' from `mcgen_amd.metrics.GanScorer` (streaming float64 accumulators on the
    device, csrc/score_ops.hip) and the checkpoint is copied to <model_tag>_best.pt whenever the InceptionScore improves
    (train_gan.py:29-31,119-122).  Otherwise -- CIFAR-10, whose IS / FID need downloaded inception_v3 weights, or a missing
    classifier file -- it logs the pixel statistics of the generated set under 'test/GeneratedMean', 'test/GeneratedStd': a
    STAND-IN, named as such in its log line, with no pivot (the `cgan` baseline's latest checkpoint is then its best);
  * the checkpoint is the reference's dict INCLUDING `scheduler_dict` (torch MultiStepLR state, train_gan.py:239-240) and the
    pickled `logger.Logger`, so `--resume_mode 1` of the reference's own driver can read a file written here;
  * --ema_decay D (default 0: off) keeps an exponential moving average of the generator's weights and BatchNorm running
    statistics (trainer.FusedEMA, csrc/ema_ops.hip), updated behind every generator step; --ema_start K copies instead of
    averaging for the first K generator updates.  test() then runs on the averaged generator (metric names unchanged), and
    the checkpoint gains one top-level key, 'generator_ema'; `model_dict` keeps the live weights.  The reference has none.
  * cfg['loss_type'] ('Hinge', train_gan.py:55) is a flag here, --loss_type {Hinge,BCE} (compat/_flags.py): both engines
    take it (train_gan.py:148-156,168-174) and it lands in the checkpoint's cfg; the model tag has no loss in it.
  * --lecam_lambda L (with --lecam_decay, --lecam_start; --engine fused only) adds the LeCam regulariser to the discriminator
    loss (trainer.FusedLeCam): the checkpoint gains one top-level key, 'lecam', and the epoch's info block
    one line with the anchors and r_t = mean sign(D(real)).  Off (the default) nothing differs.  The reference has none.
"""
import argparse
import os
import shutil
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _path  # noqa: F401,E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import models  # noqa: E402  (the compat shim: mcgen_amd's module trees under the reference's names)
import data as data_shim  # noqa: E402
from _flags import pop_ema_flags, pop_lecam_flags, pop_loss_type_flags, pop_optimizer_flags  # noqa: E402
from config import cfg  # noqa: E402
from data import fetch_dataset, make_data_loader  # noqa: E402
from logger import Logger  # noqa: E402
from utils import process_control, process_dataset, save, load  # noqa: E402


def parse():
    optimizer_flags = pop_optimizer_flags()                  # --optimizer_name / --momentum (compat/_flags.py)
    ema_flags = pop_ema_flags()                              # --ema_decay / --ema_start: the averaged generator (off at 0)
    loss_flags = pop_loss_type_flags()                       # --loss_type {Hinge,BCE}
    lecam_flags = pop_lecam_flags()                          # --lecam_lambda / --lecam_decay / --lecam_start (off at 0)
    ap = argparse.ArgumentParser(description='cfg')
    for k in cfg:                                            # train_gan.py:19-24: every cfg key is a flag
        if isinstance(cfg[k], (str, int, float)) or cfg[k] is None:
            ap.add_argument(f'--{k}', default=cfg[k], type=type(cfg[k]) if cfg[k] is not None else str)
    ap.add_argument('--control_name', default=None, type=str)
    ap.add_argument('--engine', default='fused', choices=['fused', 'autograd'])
    ap.add_argument('--synthetic_size', default=1024, type=int, help='images in the synthetic train set')
    ap.add_argument('--output_dir', default='./output')
    ap.add_argument('--generate_per_mode', default=None, type=int)
    a = vars(ap.parse_args())
    extra = {k: a.pop(k) for k in ('engine', 'synthetic_size', 'output_dir', 'generate_per_mode')}
    extra.update(ema_flags)
    extra.update(lecam_flags)
    for k in list(a):
        if k in cfg or k == 'control_name':
            cfg[k] = a[k]
    if cfg.get('control_name') == 'None':                    # train_gan.py:26-27: the baselines take no control
        cfg['control'] = {}
        cfg['control_name'] = ''
    elif cfg.get('control_name'):
        cfg['control'] = {'controller_rate': cfg['control_name'].split('_')[0]}
    cfg['optimizer_name'] = 'Adam'                           # train_gan.py:32
    cfg.update(optimizer_flags)
    cfg['loss_type'] = 'Hinge'                               # train_gan.py:55
    cfg.update(loss_flags)
    return extra


def model_tag(seed):
    """<seed>_<data>_<subset>_<model>[_<control>] (train_gan.py:57-59; empty parts dropped)."""
    control = cfg.get('control_name') or cfg['control'].get('controller_rate', '')
    return '_'.join(x for x in [str(seed), cfg['data_name'], cfg['subset'], cfg['model_name'], control] if x)


def make_model():
    """models.<model_name>() for the GANs this driver trains (train_gan.py:76)."""
    if cfg['model_name'] not in ('mcgan', 'cgan'):
        raise ValueError('Not valid model name')
    return getattr(models, cfg['model_name'])()


def make_optimizer(model, lr, betas):                        # train_gan.py:222-236
    name = cfg['optimizer_name']
    if name == 'SGD':
        return torch.optim.SGD(model.parameters(), lr=lr, momentum=cfg['momentum'], weight_decay=cfg['weight_decay'])
    if name == 'RMSprop':
        return torch.optim.RMSprop(model.parameters(), lr=lr, momentum=cfg['momentum'], weight_decay=cfg['weight_decay'])
    if name == 'Adam':
        return torch.optim.Adam(model.parameters(), lr=lr, weight_decay=cfg['weight_decay'], betas=betas)
    if name == 'Adamax':
        return torch.optim.Adamax(model.parameters(), lr=lr, weight_decay=cfg['weight_decay'], betas=betas)
    raise ValueError('Not valid optimizer name')


def make_trainer(model, lr, betas, world=1, ema_decay=0.0, ema_start=0, lecam=None):
    """The fused counterpart of make_optimizer: GraphedGANTrainer builds cfg['optimizer_name'] for both networks, the
    averaged generator when ema_decay > 0, and the LeCam regulariser when `lecam` (pop_lecam_flags' dict) has lambda > 0."""
    from mcgen_amd.trainer import GraphedGANTrainer
    return GraphedGANTrainer(model, cfg['classes_size'], lr=lr, betas=betas, optimizer=cfg['optimizer_name'],
                             momentum=cfg['momentum'], weight_decay=cfg['weight_decay'], ema_decay=ema_decay, ema_start=ema_start,
                             loss_type=cfg['loss_type'], **(lecam or {}), dist_group=(torch.distributed.group.WORLD if world > 1 else None), world_size=world)


def make_scheduler(optimizer):                               # train_gan.py:239-256 ('None' and the epoch-stepped ones)
    name = cfg.get('scheduler_name', 'None')
    if name == 'None':
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[65535])
    if name == 'StepLR':
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=cfg['step_size'], gamma=cfg['factor'])
    if name == 'MultiStepLR':
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=cfg['milestones'], gamma=cfg['factor'])
    if name == 'ExponentialLR':
        return torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.99)
    if name == 'CosineAnnealingLR':
        return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=int(cfg['num_epochs']))
    raise ValueError('Not valid scheduler name')


from _single import FusedSchedule as _FusedScheduleBase  # noqa: E402


class FusedSchedule(_FusedScheduleBase):
    """compat/_single.FusedSchedule with this driver's scheduler table (train_gan.py:239-256)."""

    def __init__(self, fused):
        super().__init__(fused, make=make_scheduler)


def train_autograd(loader, model, optimizer, epoch):
    """train_gan.py:128-194 on the module surface."""
    model.train(True)
    last = None
    for i, input in enumerate(loader):
        img, label = input['img'], input['label']
        for _ in range(cfg['iter']['discriminator']):
            optimizer['discriminator'].zero_grad(); optimizer['generator'].zero_grad()
            d_x = model.discriminate(img, label)
            generated = model.generate(label)
            d_gz = model.discriminate(generated.detach(), label)
            if cfg['loss_type'] == 'BCE':                    # train_gan.py:148-156
                d_loss = F.binary_cross_entropy_with_logits(d_x, torch.ones((img.size(0), 1), device=cfg['device'])) + \
                    F.binary_cross_entropy_with_logits(d_gz, torch.zeros((img.size(0), 1), device=cfg['device']))
            elif cfg['loss_type'] == 'Hinge':
                d_loss = F.relu(1.0 - d_x).mean() + F.relu(1.0 + d_gz).mean()
            else:
                raise ValueError('Not valid loss type')
            d_loss.backward()
            optimizer['discriminator'].step()
        for _ in range(cfg['iter']['generator']):
            optimizer['discriminator'].zero_grad(); optimizer['generator'].zero_grad()
            generated = model.generate(label)
            d_gz2 = model.discriminate(generated, label)
            if cfg['loss_type'] == 'BCE':                    # train_gan.py:168-174
                g_loss = F.binary_cross_entropy_with_logits(d_gz2, torch.ones((img.size(0), 1), device=cfg['device']))
            elif cfg['loss_type'] == 'Hinge':
                g_loss = -d_gz2.mean()
            else:
                raise ValueError('Not valid loss type')
            g_loss.backward()
            optimizer['generator'].step()
        last = (float(d_loss), float(g_loss))
    return last


def make_scorer(dataset):
    """The epoch's IS / FID scorer (train_gan.py:208-216 through metrics.py:44-161), or None where only the stand-in can be
    logged: a dataset the reference scores with inception_v3, or no trained classifier at the reference's location."""
    from mcgen_amd.data import normalize_uint8
    from mcgen_amd.metrics import GanScorer, classifier_checkpoint_path
    if cfg['data_name'] not in ('COIL100', 'Omniglot') or not os.path.exists(classifier_checkpoint_path(cfg['data_name'], cfg['subset'])):
        return None
    real = (normalize_uint8(part).contiguous() for part in dataset['train'].img.split(512))
    return GanScorer(cfg['data_name'], real, subset=cfg['subset'], device=cfg['device'])


def pivot_update(pivot, value):
    """train_gan.py:119-122: (the new pivot, whether the checkpoint becomes _best.pt).  InceptionScore is maximised, the
    comparison is strict and starts from -inf, so the first epoch always copies and a tie keeps the earlier epoch."""
    return (value, True) if pivot < value else (pivot, False)


def test(model, per_mode, logger, epoch, scorer=None):
    """train_gan.py:197-220: generate_per_mode images per class in eval mode, evaluate, log.  With a scorer the metrics
    are InceptionScore and FID, fed chunk by chunk; without one a STAND-IN (pixel mean / std of the generated set): see
    the module docstring."""
    model.train(False)
    C = torch.arange(cfg['classes_size'], device=cfg['device']).repeat(per_mode)
    chunks = C.split(min(500, C.numel()))
    if scorer is not None:
        with torch.no_grad():
            evaluation = scorer.score(model.generate(c) for c in chunks)       # consumed chunk by chunk, never concatenated
        model.train(True)
        logger.append(evaluation, 'test')
        logger.append({'info': ['Model: {}'.format(cfg['model_tag']), 'Test Epoch: {}({:.0f}%)'.format(epoch, 100.)]}, 'test', mean=False)
        logger.write('test', cfg['metric_name']['test'])
        return dict(evaluation, n=int(C.numel()))
    with torch.no_grad():
        outs = [model.generate(c) for c in chunks]
        generated = (torch.cat(outs) + 1) / 2 * 255
    model.train(True)
    stats = {'GeneratedMean': float(generated.mean()), 'GeneratedStd': float(generated.std())}
    logger.append(stats, 'test')
    logger.append({'info': ['Model: {}'.format(cfg['model_tag']), 'Test Epoch: {}({:.0f}%)'.format(epoch, 100.),
                            '[stand-in metrics: IS / FID need inception_v3 weights]']}, 'test', mean=False)
    logger.write('test', list(stats))
    return dict(stats, n=int(generated.shape[0]))


def run():
    extra = parse()
    process_control()
    from mcgen_amd import dist as mdist
    from mcgen_amd.checkpoint import make_checkpoint, resume
    rank, world, local = mdist.init_from_env() if int(cfg['world_size']) > 1 else (0, 1, 0)
    cfg['device'] = f'cuda:{local}'
    torch.cuda.set_device(local)
    seed = int(cfg['init_seed'])
    torch.manual_seed(seed); torch.cuda.manual_seed(seed)    # train_gan.py:54-55
    cfg['iter'] = {'generator': 1, 'discriminator': 5}       # train_gan.py:30-31
    cfg['pivot_metric'], cfg['pivot'] = 'InceptionScore', -float('inf')                                  # train_gan.py:29-31
    cfg['metric_name'] = {'train': ['Loss', 'Loss_D', 'Loss_G'], 'test': ['InceptionScore', 'FID']}
    cfg['model_tag'] = model_tag(seed)
    print(f'Experiment: {cfg["model_tag"]}')
    data_shim._SYNTHETIC['train'] = extra['synthetic_size']
    dataset = fetch_dataset(cfg['data_name'], cfg['subset'])                   # train_gan.py:71-73
    process_dataset(dataset['train'])
    loader = make_data_loader(dataset)['train']
    loader.drop_last = True
    model = make_model().to(cfg['device'])
    if cfg.get('compute_dtype') == 'bfloat16':
        model.set_compute_dtype(torch.bfloat16)
    if world > 1:
        mdist.broadcast_tensors(list(model.parameters()) + list(model.buffers()))
        # every rank built the same model from the same seed; from here on the ranks must differ: their own shard of a
        # common per-epoch permutation (DeviceLoader.set_shard = what DistributedSampler does) and their own latents
        torch.manual_seed(seed + rank); torch.cuda.manual_seed(seed + rank)
        loader.set_shard(rank, world, seed)
    path = os.path.join(extra['output_dir'], 'model', f'{cfg["model_tag"]}_checkpoint.pt')
    if extra['engine'] == 'fused':
        tr = make_trainer(model, 2e-4, (0.5, 0.999), world, extra['ema_decay'], extra['ema_start'],
                          {k: extra[k] for k in ('lecam_lambda', 'lecam_decay', 'lecam_start')} if extra['lecam_lambda'] else None)
        optimizer = {'generator': tr.opt_g, 'discriminator': tr.opt_d}
    else:
        if extra['ema_decay']:
            raise ValueError('Not valid engine: --ema_decay needs --engine fused')
        if extra['lecam_lambda']:
            raise ValueError('Not valid engine: --lecam_lambda needs --engine fused')
        tr = None
        optimizer = {'generator': make_optimizer(model.generator, 2e-4, (0.5, 0.999)),
                     'discriminator': make_optimizer(model.discriminator, 2e-4, (0.5, 0.999))}
    scheduler = {k: (FusedSchedule(o) if tr is not None else make_scheduler(o)) for k, o in optimizer.items()}
    ema = tr.ema if tr is not None else None                 # None: no averaged generator, the checkpoint keeps today's keys
    lecam = tr.lecam if tr is not None else None             # None: no regulariser, log and checkpoint as they were
    last_epoch, logger = 1, None
    if int(cfg['resume_mode']) == 1 and os.path.exists(path):                  # train_gan.py:80-81,258-282
        last_epoch, logger = resume(path, model, optimizer, scheduler, ema=ema, lecam=lecam)
        if tr is not None:
            tr.geng.refresh_images(force=True)
        print(f'Resume from {last_epoch}')
    if logger is None:
        logger = Logger(os.path.join(extra['output_dir'], 'runs', 'train_{}_{}'.format(cfg['model_tag'], time.strftime('%b%d_%H-%M-%S'))))
    per_mode = extra['generate_per_mode'] or cfg['generate_per_mode']
    scorer = make_scorer(dataset)
    for epoch in range(last_epoch, int(cfg['num_epochs']) + 1):
        t0 = time.time()
        logger.safe(True)
        if tr is not None:
            last = None
            for input in loader:
                if tr._graphs is None:
                    tr.capture(input['img'], input['label'])
                dl, gl = tr.train_iteration(input['img'], input['label'])
                last = (dl, gl)
            last = (float(last[0]), float(last[1]))
        else:
            last = train_autograd(loader, model, optimizer, epoch)
        n_img = len(loader) * loader.batch_size                 # this rank's share of the epoch (the loader is sharded)
        logger.append({'Loss_D': last[0], 'Loss_G': last[1], 'Loss': abs(last[0] - last[1])}, 'train', n=n_img)   # train_gan.py:177-180
        rate = n_img * world / (time.time() - t0)               # samples consumed by all ranks / wall time
        info = ['Model: {}'.format(cfg['model_tag']), 'Train Epoch: {}(100%)'.format(epoch), '{:.0f} images/s'.format(rate)]
        if lecam is not None:                                # read here, at the log interval: no per-step synchronisation
            (a_r, a_f), r_t = lecam.anchors(), lecam.stats()['r_t']
            info.append('LeCam: a_R {:.4f} a_F {:.4f} r_t {:.3f}'.format(float(a_r), float(a_f), float(r_t)))
        logger.append({'info': info}, 'train', mean=False)
        if rank == 0:
            logger.write('train', ['Loss', 'Loss_D', 'Loss_G'])
        if ema is not None:
            with tr.ema_weights():                           # scorer and stand-in alike describe the averaged generator
                test(model, per_mode, logger, epoch, scorer)
        else:
            test(model, per_mode, logger, epoch, scorer)
        for sch in scheduler.values():                                         # train_gan.py:105-106
            sch.step()
        logger.safe(False)
        if rank == 0:
            save(make_checkpoint(model, optimizer, epoch + 1, cfg, scheduler=scheduler, logger=logger, ema=ema, lecam=lecam), path)   # train_gan.py:111-119
            if scorer is not None:                                             # train_gan.py:119-122
                cfg['pivot'], best = pivot_update(cfg['pivot'], logger.mean['test/{}'.format(cfg['pivot_metric'])])
                if best:
                    shutil.copy(path, path[:-len('_checkpoint.pt')] + '_best.pt')
            elif cfg['model_name'] == 'cgan':
                # the stand-in metric has no pivot, so the baseline's latest checkpoint is its best (what compat/generate.py reads)
                shutil.copy(path, path[:-len('_checkpoint.pt')] + '_best.pt')
        logger.reset()
    logger.safe(False)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    run()
