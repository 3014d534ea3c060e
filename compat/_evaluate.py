"""What the reference's five per-model evaluation drivers share (src/test_vae.py, test_glow.py, test_pixelcnn.py, test_vqvae.py
and test_classifier.py are near-clones): resume <model_tag>_best.pt, run the TRAIN loader once in eval mode under no_grad
(test_vae.py:46,54), fold the per-batch metrics into a Logger, print the 'test' line and save {'cfg', 'epoch', 'logger'} to
output/result/<model_tag>.pt (test_vae.py:56-57) -- the file the paper's numbers are read from.  compat/test_vae.py and its
siblings are the model-specific overrides on top of this, each citing the lines it restates; the command line and the *_best.pt
loading are create.py's (`main`, `load_models_with_epoch`).

  --metrics device (default): the running means are summed on the device by mcgen_amd.evaluate.DeviceEvaluator -- no host
      synchronisation per batch -- and reach the Logger once, with n = the number of samples counted;
  --metrics host: the reference's loop itself, `Metric.evaluate` and `Logger.append` per batch as in _single.Driver.test.
Both include the reference's trailing `logger.append(evaluation, 'test')` (the last batch once more with n = 1, test_vae.py:72)
where the reference has it.  --batch and --synthetic_size as in the train drivers."""
import datetime

import torch

import _single  # noqa: F401  (sys.path)
from _single import cfg
from create import load_models_with_epoch, main as create_main
from data import make_data_loader
from generate import _pop_flag
from logger import Logger
from metrics import Metric
from utils import save, save_img, to_device


class EvalDriver:
    """One of test_vae.py / test_glow.py / test_pixelcnn.py / test_vqvae.py / test_classifier.py."""
    metric_names = ['Loss']
    trailing_append = True                                # test_classifier.py has no `logger.append(evaluation, 'test')`
    grids = False                                         # test_vae.py:76-77: input_ / output_ grids of the first 100 images
    runs_prefix = 'test'                                  # output/runs/<prefix>_<tag>_<time> (test_pixelcnn.py:55 says 'train')

    def __init__(self):
        self.mode = 'device'

    # ---- hooks -----------------------------------------------------------------------------------------------------------
    def prepare(self, input, ae):                         # test_pixelcnn.py:74-75: img -> code map
        return input

    def reconstruct(self, model, input, output):          # test_glow.py:77-79
        return output

    # ---- test_vae.py:60-78 -------------------------------------------------------------------------------------------------
    def test(self, loader, model, ae, logger, epoch):
        names = self.metric_names
        with torch.no_grad():
            model.train(False)
            if ae is not None:
                ae.train(False)
            input = output = None
            if self.mode == 'device':
                from mcgen_amd.evaluate import DeviceEvaluator
                ev = DeviceEvaluator(names, cfg['device'])
                for input in loader:
                    input = self.prepare(to_device(input, cfg['device']), ae)
                    # the loader's images are NCHW views of NHWC storage: laid out once here, for the model and the kernels alike
                    input['img'] = input['img'].contiguous()
                    output = model(input)
                    ev.update(input, output)
                if self.trailing_append:
                    ev.repeat_last()
                result, last = ev.fetch()                 # the pass's one device-to-host copy
                logger.append(result, 'test', ev.count)
                for k, v in last.items():                 # what the per-batch appends leave in the tracker
                    logger.tracker['test/{}'.format(k)] = v
            else:
                metric = Metric()
                evaluation = None
                for input in loader:
                    input_size = input['img'].size(0)
                    input = self.prepare(to_device(input, cfg['device']), ae)
                    output = model(input)
                    evaluation = metric.evaluate(names, input, output)
                    logger.append(evaluation, 'test', input_size)
                if self.trailing_append:
                    logger.append(evaluation, 'test')
            info = {'info': ['Model: {}'.format(cfg['model_tag']), 'Test Epoch: {}({:.0f}%)'.format(epoch, 100.)]}
            logger.append(info, 'test', mean=False)
            logger.write('test', names)
            if self.grids:
                output = self.reconstruct(model, input, output)
                save_img(input['img'][:100], './output/vis/input_{}.png'.format(cfg['model_tag']), range=(-1, 1))
                save_img(output['img'][:100], './output/vis/output_{}.png'.format(cfg['model_tag']), range=(-1, 1))

    # ---- test_vae.py:40-57 -------------------------------------------------------------------------------------------------
    def run_experiment(self, extra):
        if extra['batch']:
            cfg['batch_size'] = dict(cfg['batch_size'], train=extra['batch'])
        model, ae, dataset, last_epoch = load_models_with_epoch(extra)          # the epoch of <model_tag>_best.pt (test_vae.py:49)
        loader = make_data_loader(dataset)['train']
        now = datetime.datetime.now().strftime('%b%d_%H-%M-%S')
        logger = Logger('output/runs/{}_{}_{}'.format(self.runs_prefix, cfg['model_tag'], now))
        logger.safe(True)
        self.test(loader, model, ae, logger, last_epoch)
        logger.safe(False)
        save({'cfg': dict(cfg), 'epoch': last_epoch, 'logger': logger}, './output/result/{}.pt'.format(cfg['model_tag']))

    def main(self, models):
        mode = _pop_flag('--metrics') or 'device'
        if mode not in ('device', 'host'):
            raise ValueError('Not valid metrics mode: {} (device or host)'.format(mode))
        self.mode = mode

        def run(extra):
            if cfg['model_name'] not in models:
                raise ValueError('Not valid model name')
            self.run_experiment(extra)
        create_main(run, {'metric_name': {'train': list(self.metric_names), 'test': list(self.metric_names)}})
