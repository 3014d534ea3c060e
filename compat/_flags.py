"""Command-line flags for cfg keys that only process_control creates: they are popped from argv before the shared parser
sees it and applied to cfg after process_control has built its table.  No imports beyond the standard library, so every
driver (and a test) can use it."""
import sys

GLOW_KEYS = ('affine', 'conv_lu')                         # cfg['glow'] keys of the reference's table (utils.py:183-184)
_REFUSED = {'affine': 'Not valid coupling: only the affine form (cfg glow.affine = True) is built',
            'conv_lu': 'Not valid invertible conv: only the LU form (cfg glow.conv_lu = True) is built'}


def pop_flag(name, argv=None):
    """Remove `--name V` / `--name=V` from argv; -> V or None."""
    argv = sys.argv if argv is None else argv
    for i, a in enumerate(argv):
        if a == name and i + 1 < len(argv):
            v = argv[i + 1]
            del argv[i:i + 2]
            return v
        if a.startswith(name + '='):
            del argv[i]
            return a.split('=', 1)[1]
    return None


OPTIMIZERS = ('SGD', 'RMSprop', 'Adam', 'Adamax')         # train_gan.py:222-236, train_vae.py:151-165


def pop_optimizer_flags(argv=None):
    """--optimizer_name {SGD,RMSprop,Adam,Adamax} / --momentum M -> {cfg key: value} of the flags given.  The drivers set
    cfg['optimizer_name'] = 'Adam' after their parser ran, as the reference's do (train_vae.py:32, train_gan.py:32), and
    cfg['momentum'] parses as the int its default is: the two flags are popped first and applied (cfg.update) last."""
    out = {}
    v = pop_flag('--optimizer_name', argv)
    if v is not None:
        if v not in OPTIMIZERS:
            raise ValueError('Not valid optimizer name')
        out['optimizer_name'] = v
    v = pop_flag('--momentum', argv)
    if v is not None:
        out['momentum'] = float(v)
    return out


LOSS_TYPES = ('Hinge', 'BCE')                             # train_gan.py:148-156,168-174


def pop_loss_type_flags(argv=None):
    """--loss_type {Hinge,BCE} -> {'loss_type': value} if given.  The driver sets cfg['loss_type'] = 'Hinge' after its
    parser ran, as the reference does (train_gan.py:55): the flag is popped first and applied (cfg.update) last."""
    v = pop_flag('--loss_type', argv)
    if v is None:
        return {}
    if v not in LOSS_TYPES:
        raise ValueError('Not valid loss type')
    return {'loss_type': v}


def pop_ema_flags(argv=None):
    """--ema_decay D / --ema_start K (train_gan.py) -> {'ema_decay': float, 'ema_start': int}; 0 / 0 when not given: no
    averaged generator.  K counts generator updates: the average copies the parameters until K updates are done."""
    d, k = pop_flag('--ema_decay', argv), pop_flag('--ema_start', argv)
    out = {'ema_decay': 0.0 if d is None else float(d), 'ema_start': 0 if k is None else int(k)}
    if not 0.0 <= out['ema_decay'] < 1.0 or out['ema_start'] < 0:
        raise ValueError('Not valid --ema_decay / --ema_start: decay in [0, 1), start >= 0')
    return out


def pop_lecam_flags(argv=None):
    """--lecam_lambda L / --lecam_decay D / --lecam_start K (train_gan.py) -> {'lecam_lambda': float, 'lecam_decay': float,
    'lecam_start': int}; 0 / 0.99 / 0 when not given: no regulariser.  K counts discriminator updates: the term is off
    until K updates are done, the anchors move from the first."""
    lam, d, k = pop_flag('--lecam_lambda', argv), pop_flag('--lecam_decay', argv), pop_flag('--lecam_start', argv)
    out = {'lecam_lambda': 0.0 if lam is None else float(lam), 'lecam_decay': 0.99 if d is None else float(d),
           'lecam_start': 0 if k is None else int(k)}
    if not 0.0 <= out['lecam_lambda'] < float('inf') or not 0.0 <= out['lecam_decay'] < 1.0 or out['lecam_start'] < 0:
        raise ValueError('Not valid --lecam_lambda / --lecam_decay / --lecam_start: lambda >= 0, decay in [0, 1), start >= 0')
    if out['lecam_lambda'] == 0 and (d is not None or k is not None):
        raise ValueError('Not valid --lecam_decay / --lecam_start: they go with --lecam_lambda > 0')
    return out


def pop_use_ema(argv=None):
    """--use_ema {True,False} (the sampling drivers) -> bool, False when not given."""
    v = pop_flag('--use_ema', argv)
    if v is None:
        return False
    if v not in ('True', 'False'):
        raise ValueError('Not valid --use_ema: {} (True or False)'.format(v))
    return v == 'True'


def check_use_ema(use_ema, model_name):
    """--use_ema is a flag of the GAN models: only compat/train_gan.py keeps an averaged generator."""
    if use_ema and model_name not in ('mcgan', 'cgan'):
        raise ValueError('Not valid model name: --use_ema is a flag of mcgan / cgan')


def pop_glow_flags(argv=None):
    """--glow_affine {True,False} / --glow_conv_lu {True,False} -> {key: bool} of the flags given (none: the table stays)."""
    out = {}
    for key in GLOW_KEYS:
        v = pop_flag('--glow_' + key, argv)
        if v is None:
            continue
        if v not in ('True', 'False'):
            raise ValueError('Not valid --glow_{}: {} (True or False)'.format(key, v))
        out[key] = v == 'True'
    return out


def apply_glow_flags(cfg, flags):
    """After process_control: set the popped keys in cfg['glow'].  MCGlow builds both values of each (mcglow.py:146,182-185);
    the CGlow baseline only the table's, so a False is refused for it with its constructor's message."""
    if not flags:
        return
    if 'glow' not in cfg.get('model_name', ''):
        raise ValueError('Not valid model name: --glow_affine / --glow_conv_lu are flags of mcglow')
    if cfg['model_name'] != 'mcglow':
        for key in GLOW_KEYS:
            if flags.get(key) is False:
                raise ValueError(_REFUSED[key])
    cfg['glow'] = dict(cfg['glow'], **flags)
