#!/usr/bin/env python3
"""Counterpart of the reference's tools/train.py (same CLI, YAML schema and work-dir layout) on the
MI355X hot path.

    python tools/train.py <config.yml> [--resume_from weights.npz] [--synthetic N_CLASSES]

Triplet mode runs the fused step (one forward, on-GPU distance matrix + mining + hinge, backward,
optimizer); siamese mode trains SiameseNet with contrastive_loss.  Per-epoch schedule as the reference:
lr0 * decay^floor(epoch/step) (train.py:80-81), ReduceLROnPlateau(0.1, patience 4) (:82-83),
EarlyStopping(patience 10) (:84-86), best-only checkpoints weights/epoch_XXX.npz (:87-90).
Multi-GPU: launch with torchrun; classes are sharded per rank and gradients all-reduced over RCCL.
GENERATOR.negatives_selection_mode 'proxy_anchor' / 'proxy_softmax' train the backbone together with one learnable proxy per
class (train_step.ProxyTrainer on the feeder's labelled batches); the proxies are checkpointed as proxies/epoch_XXX.npz.
'soft_triple' / 'arcface' do the same with GENERATOR.proxy_loss.centers learnable centres per class (SoftTriple, sub-centre ArcFace).
GENERATOR.xbm: {size, weight, start_iteration, loss, <that loss's parameters>} adds a cross-batch memory (train_step.XbmTrainer,
embeddingnet_amd/xbm.py) to any triplet-mode negatives_selection_mode but the proxy ones: the loss of the batch against the detached
embeddings of the last `size` samples, `weight` times, from step `start_iteration` on; `xbm_filled` and the kept pairs are logged
per epoch.  Each rank keeps its own memory; it is not checkpointed, after --resume_from it refills.
GENERATOR.circle_loss: {m, gamma} sets Circle loss's parameters for negatives_selection_mode 'circle' (and `loss: 'circle'` with the
same two keys under GENERATOR.xbm scores the memory with it); the violating anchors are logged per epoch.
GENERATOR.margin_loss: {beta, alpha, cutoff, nonzero_loss_cutoff} sets the margin loss's boundary and margin and the sampler's two
cutoffs for negatives_selection_mode 'distance_weighted' (Wu et al., ICCV 2017); the active pairs per step are logged per epoch.
TRAIN.weight_averaging: {mode, decay, warmup, start_epoch, update_every, evaluate} keeps an exponential moving average ('ema') or a
stochastic weight average ('swa') of the model — and of the proxies in the proxy modes — by one more launch per step
(embeddingnet_amd/weight_average.py; the keys: utils.check_weight_averaging).  With evaluate 'averaged' (the default) everything
computed for validation — val_loss, the retrieval, MAP, NMI and verification values, and with them monitor, plateau, early stop and
best checkpoint — is computed with the averages in the model, from the first update on; the epoch line adds `averaged <updates>`.
weights/epoch_XXX.npz stays the live model; the averages go to averaged/epoch_XXX.npz beside it, in the same format (load_model
serves it for inference), and the update count into the optimizer state; --resume_from restores both.
`--synthetic` swaps the file loader for an in-memory synthetic dataset (no dataset ships with the repo).
"""
import argparse
import os
import sys

BASE_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(BASE_DIR)
sys.path.insert(0, ROOT_DIR)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from embedding_net.models import TripletNet, SiameseNet  # noqa: E402
from embedding_net.utils import parse_params  # noqa: E402
from embedding_net.losses_and_accuracies import contrastive_loss, triplet_loss, accuracy  # noqa: E402
from embeddingnet_amd.datagenerators import (ENDataLoader, SyntheticDataLoader, TripletsDataGenerator,  # noqa: E402
                                             SimpleTripletsDataGenerator, SiameseDataGenerator)
from embeddingnet_amd.parallel import (GradReducer, all_reduce_mean, average_buffers, broadcast_model,  # noqa: E402
                                       init_distributed, shard_classes)
from embeddingnet_amd.train_step import TripletTrainer  # noqa: E402


def parse_args():
    parser = argparse.ArgumentParser(description='Train an embedding network')
    parser.add_argument('config', help='model config file path')
    parser.add_argument('--resume_from', help='the checkpoint file to resume from')
    parser.add_argument('--synthetic', type=int, default=0, help='use N synthetic classes instead of DATALOADER')
    parser.add_argument('--max_epochs', type=int, default=None, help='cap TRAIN.n_epochs (smoke runs)')
    return parser.parse_args()


def create_save_folders(params):
    work_dir_path = os.path.join(params['work_dir'], params['project_name'])
    paths = {k: os.path.join(work_dir_path, v) for k, v in
             dict(weights='weights/', pretrained='pretraining_model/weights/', encodings='encodings/', plots='plots/',
                  tf_log='tf_log/', pretrained_log='pretraining_model/tf_log/').items()}
    for p in [work_dir_path] + list(paths.values()):
        os.makedirs(p, exist_ok=True)
    return paths


def _optimizer_state_path(weights_path):
    """<project>/weights/epoch_007.npz -> <project>/optimizer/epoch_007.npz (the weights folder holds weight files only)."""
    d, f = os.path.split(os.path.abspath(weights_path))
    return os.path.join(os.path.dirname(d), 'optimizer', f)


class Plateau:
    """The three monitor-driven Keras callbacks of the reference (train.py:82-90), each with its own state as in Keras:
      ReduceLROnPlateau(factor .1, patience 4): `min_delta` 1e-4 (Keras default, mode 'min': an epoch improves only if
        value < best - 1e-4), cooldown 0, min_lr 0;  after 4 epochs without that improvement the learning rate is
        multiplied by 0.1 and the wait restarts;
      EarlyStopping(patience 10, min_delta 0): stop after 10 epochs without value < best;
      ModelCheckpoint(save_best_only): save when value < best.
    update(value, lr) -> (save checkpoint?, stop?, lr after the epoch).
    NB the reference ALSO installs LearningRateScheduler(lambda epoch: lr0 * decay ** floor(epoch / step)) — a one-argument
    schedule, which Keras applies at every epoch BEGIN by setting the optimizer's lr outright.  It therefore overwrites
    whatever ReduceLROnPlateau set at the previous epoch end: in the reference the plateau reduction never reaches a
    training step (it only shows in the log).  main() reproduces that order; `persistent=True` is this port's opt-in
    (TRAIN.plateau_persistent) to let reductions accumulate as a multiplier on the schedule instead."""

    def __init__(self, factor=0.1, patience=4, min_delta=1e-4, stop_patience=10, persistent=False):
        self.factor, self.patience, self.min_delta, self.stop_patience = factor, patience, min_delta, stop_patience
        self.persistent, self.scale = persistent, 1.0
        self.rl_best, self.rl_wait = float('inf'), 0          # ReduceLROnPlateau
        self.es_best, self.es_wait = float('inf'), 0          # EarlyStopping
        self.best = float('inf')                              # ModelCheckpoint

    def update(self, value, lr=None):
        if value < self.rl_best - self.min_delta:
            self.rl_best, self.rl_wait = value, 0
        else:
            self.rl_wait += 1
            if self.rl_wait >= self.patience:
                self.rl_wait = 0
                self.scale *= self.factor
                if lr is not None:
                    lr = lr * self.factor
                    print(f'ReduceLROnPlateau reducing learning rate to {lr:g}.', flush=True)
        if value < self.es_best:
            self.es_best, self.es_wait = value, 0
        else:
            self.es_wait += 1
        save = value < self.best
        if save:
            self.best = value
        return save, self.es_wait >= self.stop_patience, lr


def apply_gpu_ids(gpu_ids):
    """GENERAL.gpu_ids (reference train.py:121-133: CUDA_VISIBLE_DEVICES + n_gpu): the listed devices become the
    visible ones; with more than one id and no launcher around us, re-run this script as one process per listed GPU
    under torch.distributed.run (the data-parallel world) and exit with its status.  Must run before the GPU is touched."""
    if not gpu_ids:
        return
    ids = [s.strip() for s in str(gpu_ids).split(',') if s.strip()]
    if 'WORLD_SIZE' in os.environ:                    # already under torchrun: the launcher decided the world
        if int(os.environ['WORLD_SIZE']) != len(ids):
            print(f"GENERAL.gpu_ids lists {len(ids)} devices but WORLD_SIZE={os.environ['WORLD_SIZE']}: using the launcher's world")
        return
    os.environ.setdefault('HIP_VISIBLE_DEVICES', ','.join(ids))
    print(f'Using gpu ids: {",".join(ids)}')
    if len(ids) > 1:
        # one process per listed GPU, started and WATCHED by embeddingnet_amd/launch.py: a rank that dies ends the world at
        # once with its exit code instead of leaving the others in a collective until the process-group timeout
        from embeddingnet_amd import launch
        sys.exit(launch.spawn(len(ids), [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))


def device_augmentations(cfg, synthetic=0, rank=0):
    """GENERATOR.device_augmentations (a preset name, an op list or 'none'; embeddingnet_amd/augment.py) -> the DeviceAugment
    of this rank's triplet training batches, or None.  Seeded from GENERATOR.augment_seed (default 0) mixed with the rank, so
    that data-parallel ranks draw differently.  Validation and encodings are never augmented; the softmax pre-training does
    not read the key.  Refused (ValueError) with --synthetic (no uint8 images to augment) and in Siamese mode."""
    from embeddingnet_amd.augment import DeviceAugment, rank_seed
    value = cfg['generator'].get('device_augmentations')
    aug = DeviceAugment.from_config(value, cfg['model']['input_shape'],
                                    rank_seed(cfg['generator'].get('augment_seed', 0), rank))
    if aug is not None and cfg['model']['mode'] == 'siamese':
        raise ValueError("GENERATOR.device_augmentations applies to triplet training batches; Siamese mode has none")
    if aug is not None and synthetic:
        raise ValueError("GENERATOR.device_augmentations augments decoded image files on the GPU; --synthetic datasets are "
                         "in-memory float arrays: drop the key or train on files")
    return aug


# The optional GENERATOR keys that set a loss's parameters: key -> {the negatives_selection_mode that reads it -> {parameter: check}}.
# A check is 'number', 'positive' (a number, and > 0), 'positive number' (the same under one message) or the tuple of allowed values.
LOSS_CONFIGS = {
    'ms_loss': {'multi_similarity': dict(alpha='number', beta='number', base='number', epsilon='number')},
    'supcon_loss': {'supcon': dict(temperature='positive number', denominator=('all', 'negatives'))},
    'proxy_loss': {'proxy_anchor': dict(alpha='positive', delta='number'), 'proxy_softmax': dict(scale='positive', margin='number')},
}
# GENERATOR.ap_loss with the ranking modes: the same validator on a table of its own, as for the modes below (ap_loss_config)
AP_LOSS_CONFIGS = {'fast_ap': dict(bins='positive'), 'smooth_ap': dict(temperature='positive number')}
# GENERATOR.circle_loss with 'circle': likewise (circle_loss_config)
CIRCLE_LOSS_CONFIGS = {'circle': dict(m='number', gamma='positive')}
# GENERATOR.margin_loss with 'distance_weighted': likewise (margin_loss_config)
MARGIN_LOSS_CONFIGS = {'distance_weighted': dict(beta='number', alpha='number', cutoff='positive', nonzero_loss_cutoff='positive')}
# GENERATOR.proxy_loss with the modes on several centres per class (ops.MULTI_PROXY_LOSS_MODES): the same validator on a table of
# their own (proxy_loss_config), so the messages about the key keep naming the two modes they always named
MULTI_PROXY_LOSS_CONFIGS = {
    'soft_triple': dict(scale='positive', margin='number', gamma='positive', tau='number', centers='positive'),
    'arcface': dict(scale='positive', margin='number', centers='positive'),
}
MULTI_PROXY_DEFAULT_CENTERS = {'soft_triple': 10, 'arcface': 1}
MS_LOSS_KEYS = tuple(LOSS_CONFIGS['ms_loss']['multi_similarity'])
SUPCON_LOSS_KEYS = tuple(LOSS_CONFIGS['supcon_loss']['supcon'])
PROXY_LOSS_KEYS = {mode: tuple(checks) for mode, checks in LOSS_CONFIGS['proxy_loss'].items()}
AP_LOSS_KEYS = {mode: tuple(checks) for mode, checks in AP_LOSS_CONFIGS.items()}
CIRCLE_LOSS_KEYS = tuple(CIRCLE_LOSS_CONFIGS['circle'])
MARGIN_LOSS_KEYS = tuple(MARGIN_LOSS_CONFIGS['distance_weighted'])
MARGIN_LOSS_DEFAULTS = dict(beta=1.2, alpha=0.2, cutoff=0.5, nonzero_loss_cutoff=1.4)


def loss_config(name, cfg, table=None):
    """GENERATOR.<name> (a key of LOSS_CONFIGS, or with `table` that table's; optional): any subset of the parameters of the mode's loss -> the trainer's
    loss_params (None without the key).  Only the key's own modes of a triplet-mode model read it: given with anything else, or
    with other parameters or a value that fails its check, it is a ValueError before training starts."""
    value = cfg['generator'].get(name)
    if value is None:
        return None
    table = LOSS_CONFIGS[name] if table is None else table
    mode = cfg['generator'].get('negatives_selection_mode')
    siamese = cfg['model']['mode'] == 'siamese'
    if siamese or mode not in table:
        raise ValueError(f"GENERATOR.{name} sets the parameters of negatives_selection_mode {' or '.join(map(repr, table))}; "
                         f"this config trains with {'the Siamese contrastive loss' if siamese else repr(mode)}: "
                         "drop the key or change the mode")
    checks = table[mode]
    if not isinstance(value, dict) or set(value) - set(checks):
        raise ValueError(f"GENERATOR.{name}: a mapping with keys out of {tuple(checks)}{f' for {mode!r}' if len(table) > 1 else ''} "
                         f"(got {value!r})")

    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float))
    if not all(number(v) for k, v in value.items() if checks[k] in ('number', 'positive')):
        raise ValueError(f"GENERATOR.{name}: every value must be a number (got {value!r})")
    out = {}
    for k, check in checks.items():
        if k not in value:
            continue
        v = value[k]
        if check == 'positive number' and not (number(v) and v > 0):
            raise ValueError(f"GENERATOR.{name}: {k} must be a positive number (got {v!r})")
        if check == 'positive' and not v > 0:
            raise ValueError(f"GENERATOR.{name}: {k} must be positive (got {v!r})")
        if isinstance(check, tuple) and v not in check:
            raise ValueError(f"GENERATOR.{name}: {k} must be {' or '.join(map(repr, check))} (got {v!r})")
        out[k] = v if isinstance(check, tuple) else float(v)
    return out


def ms_loss_config(cfg):
    return loss_config('ms_loss', cfg)


def supcon_loss_config(cfg):
    return loss_config('supcon_loss', cfg)


def _circle_m(name, out, value):
    """Circle loss's relaxation lies in [0, 1] (include/embnet.h); the validator's checks know numbers and signs only."""
    if out is not None and not 0 <= out.get('m', 0.4) <= 1:
        raise ValueError(f"GENERATOR.{name}: m must lie in [0, 1] (got {value!r})")
    return out


def circle_loss_config(cfg):
    """GENERATOR.circle_loss for 'circle': {m in [0, 1], gamma > 0}; `margin` is not used and embeddings_normalization should be
    on (the optima 1 - m and m are cosine similarities)."""
    return _circle_m('circle_loss', loss_config('circle_loss', cfg, CIRCLE_LOSS_CONFIGS), cfg['generator'].get('circle_loss'))


def margin_loss_config(cfg):
    """GENERATOR.margin_loss for 'distance_weighted': {beta, alpha >= 0, 0 < cutoff < nonzero_loss_cutoff < 2} (include/embnet.h);
    `margin` is not used and embeddings_normalization should be on (the weights are those of the unit sphere)."""
    out = loss_config('margin_loss', cfg, MARGIN_LOSS_CONFIGS)
    if out is None:
        return None
    value, full = cfg['generator']['margin_loss'], dict(MARGIN_LOSS_DEFAULTS, **out)
    if not 0 < full['cutoff'] < full['nonzero_loss_cutoff'] < 2:
        raise ValueError(f"GENERATOR.margin_loss: need 0 < cutoff < nonzero_loss_cutoff < 2 (got {value!r})")
    if full['alpha'] < 0:
        raise ValueError(f"GENERATOR.margin_loss: alpha must not be negative (got {value!r})")
    return out


def ap_loss_config(cfg):
    """GENERATOR.ap_loss for the ranking modes: {bins} with 'fast_ap', a whole number in [2, 64]; {temperature} with 'smooth_ap'."""
    out = loss_config('ap_loss', cfg, AP_LOSS_CONFIGS)
    if out is not None and 'bins' in out:
        if out['bins'] != int(out['bins']) or not 2 <= out['bins'] <= 64:
            raise ValueError(f"GENERATOR.ap_loss: bins must be a whole number in [2, 64] (got {cfg['generator']['ap_loss']!r})")
        out['bins'] = int(out['bins'])
    return out


def proxy_loss_config(cfg):
    """GENERATOR.proxy_loss for the proxy modes; with 'soft_triple' / 'arcface' checked against MULTI_PROXY_LOSS_CONFIGS, and then:
    centers a whole number in [1, 32], tau not negative, ArcFace's margin in [0, pi/2)."""
    mode = cfg['generator'].get('negatives_selection_mode')
    if mode not in MULTI_PROXY_LOSS_CONFIGS or cfg['model']['mode'] == 'siamese':
        return loss_config('proxy_loss', cfg)
    out = loss_config('proxy_loss', cfg, MULTI_PROXY_LOSS_CONFIGS)
    if out is None:
        return None
    value = cfg['generator']['proxy_loss']
    if 'centers' in out and (out['centers'] != int(out['centers']) or out['centers'] > 32):
        raise ValueError(f"GENERATOR.proxy_loss: centers, the centres per class, must be a whole number in [1, 32] (got {value!r})")
    if out.get('tau', 0.0) < 0:
        raise ValueError(f"GENERATOR.proxy_loss: tau must not be negative (got {value!r})")
    if mode == 'arcface' and not 0 <= out.get('margin', 0.5) < np.pi / 2:
        raise ValueError(f"GENERATOR.proxy_loss: margin must lie in [0, pi/2) for 'arcface' (got {value!r})")
    if 'centers' in out:
        out['centers'] = int(out['centers'])
    return out


# GENERATOR.xbm (optional): the memory's own keys, and per memory loss (ops.XBM_LOSS_MODES) that loss's parameters.
XBM_KEYS = dict(size='positive', weight='number', start_iteration='number', loss=('contrastive', 'multi_similarity', 'circle'))
XBM_LOSS_KEYS = {'contrastive': dict(margin='number'),
                 'multi_similarity': dict(alpha='positive', beta='positive', base='number', epsilon='number'),
                 'circle': dict(m='number', gamma='positive')}
XBM_DEFAULTS = dict(weight=1.0, start_iteration=0, loss='contrastive')
XBM_MODES = ('semihard', 'hardest', 'random_hard', 'batch_hard', 'batch_all', 'multi_similarity', 'supcon', 'fast_ap',
             'smooth_ap', 'circle', 'distance_weighted')


def xbm_config(cfg):
    """GENERATOR.xbm (optional) -> dict(size, weight, start_iteration, loss, params) or None, checked by loss_config: the key goes
    with every negatives_selection_mode of TripletTrainer and is refused (ValueError before training starts) with the proxy modes,
    in Siamese mode, with keys that are neither the memory's nor its loss's, and with a memory smaller than a batch."""
    value = cfg['generator'].get('xbm')
    if value is None:
        return None
    loss = value.get('loss', XBM_DEFAULTS['loss']) if isinstance(value, dict) else XBM_DEFAULTS['loss']
    checks = dict(XBM_KEYS, **XBM_LOSS_KEYS.get(loss, {}))
    LOSS_CONFIGS['xbm'] = {mode: checks for mode in XBM_MODES}
    out = dict(XBM_DEFAULTS, **loss_config('xbm', cfg))
    if out['loss'] == 'circle':
        _circle_m('xbm', out, value)
    if 'size' not in out or out['size'] != int(out['size']):
        raise ValueError(f"GENERATOR.xbm: size, the number of slots, must be a whole number (got {value!r})")
    if out['start_iteration'] != int(out['start_iteration']) or out['start_iteration'] < 0:
        raise ValueError(f"GENERATOR.xbm: start_iteration must be a whole number >= 0 (got {value!r})")
    batch = int(cfg['generator']['k_classes']) * int(cfg['generator']['k_samples'])
    if out['size'] < batch:
        raise ValueError(f"GENERATOR.xbm: a memory of {int(out['size'])} slots is smaller than a batch of {batch}")
    return dict(size=int(out['size']), weight=float(out['weight']), start_iteration=int(out['start_iteration']), loss=out['loss'],
                params={k: out[k] for k in XBM_LOSS_KEYS[out['loss']] if k in out})


def _proxies_path(weights_path):
    """<project>/weights/epoch_007.npz -> <project>/proxies/epoch_007.npz (the class proxies of the proxy losses)."""
    d, f = os.path.split(os.path.abspath(weights_path))
    return os.path.join(os.path.dirname(d), 'proxies', f)


def _averaged_path(weights_path):
    """<project>/weights/epoch_007.npz -> <project>/averaged/epoch_007.npz (the averaged weights of TRAIN.weight_averaging)."""
    d, f = os.path.split(os.path.abspath(weights_path))
    return os.path.join(os.path.dirname(d), 'averaged', f)


def build_averager(section, modules, steps_per_epoch):
    """TRAIN.weight_averaging (utils.check_weight_averaging's result) -> the WeightAverager over `modules`: epochs become steps."""
    from embeddingnet_amd.weight_average import WeightAverager
    every = steps_per_epoch if section['update_every'] == 'epoch' else section['update_every']
    kw = dict(decay=section['decay'], warmup=section['warmup']) if section['mode'] == 'ema' else {}
    return WeightAverager(modules, mode=section['mode'], start_iteration=section['start_epoch'] * steps_per_epoch,
                          update_every=every, **kw)


def save_proxies(path, head, class_names):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, proxies=head.proxies.detach().cpu().numpy(), class_names=np.asarray(list(class_names), dtype=str),
             centers_per_class=np.int64(head.centers_per_class))


def load_proxies(path, head, class_names):
    """The proxies of a checkpoint into `head`; a file for other classes (or another order of them), or with another number of
    centres per class (a file without the key has one), is refused."""
    d = np.load(path, allow_pickle=False)
    kc = int(d['centers_per_class']) if 'centers_per_class' in d.files else 1
    if kc != head.centers_per_class:
        raise ValueError(f"{path}: its centers_per_class is {kc}, this run's is {head.centers_per_class}")
    if [str(v) for v in d['class_names']] != [str(v) for v in class_names]:
        raise ValueError(f"{path}: its class_names differ from the dataset's: the proxies belong to other classes")
    if tuple(d['proxies'].shape) != tuple(head.proxies.shape):
        raise ValueError(f"{path}: proxies {tuple(d['proxies'].shape)} do not match {tuple(head.proxies.shape)}")
    with torch.no_grad():
        head.proxies.copy_(torch.from_numpy(d['proxies']).to(head.proxies.device))


MAP_MONITORS = ('val_map@r', 'val_r_precision')


def retrieval_map_config(p_train, validate):
    """TRAIN.retrieval_map (optional, default off) -> bool: after each epoch's validation, MAP@R and R-precision of the validation
    set (leave-one-out, EmbeddingNet.calculate_map_at_r) join the history as val_map@r / val_r_precision."""
    on = p_train.get('retrieval_map') or False
    if not isinstance(on, bool):
        raise ValueError(f"TRAIN.retrieval_map: true or false (got {on!r})")
    if on and not validate:
        raise ValueError("TRAIN.retrieval_map evaluates the validation set: it needs DATALOADER.validate (validation is off)")
    return on


def clustering_nmi_config(p_train, validate):
    """TRAIN.clustering_nmi (optional, default off) -> bool: after each epoch's validation, the NMI of a k-means clustering of the
    validation encodings against their classes (EmbeddingNet.calculate_clustering_metrics, as many clusters as classes, seed 0)
    joins the history as val_nmi."""
    on = p_train.get('clustering_nmi') or False
    if not isinstance(on, bool):
        raise ValueError(f"TRAIN.clustering_nmi: true or false (got {on!r})")
    if on and not validate:
        raise ValueError("TRAIN.clustering_nmi evaluates the validation set: it needs DATALOADER.validate (validation is off)")
    return on


VERIFICATION_DEFAULTS = {'fars': [1e-1, 1e-2, 1e-3], 'bins': 4096}
LOWER_IS_BETTER = ('val_eer',)                             # monitored evaluation values that improve downwards


def verification_config(p_train, validate):
    """TRAIN.verification (optional, default off) -> None or {'fars': [...], 'bins': int}: after each epoch's validation, ROC AUC,
    equal error rate and TAR@FAR over all pairs of the validation set (EmbeddingNet.calculate_verification_metrics) join the
    history as val_auc / val_eer / val_tar@far=f, f written as repr(f).  `true` takes the defaults; a mapping may set `fars`
    (each in (0, 1)) and `bins` (a power of two in [2, 4096]); any other sub-key is refused."""
    raw = p_train.get('verification')
    if raw is None or raw is False:
        return None
    if raw is True:
        raw = {}
    if not isinstance(raw, dict):
        raise ValueError(f"TRAIN.verification: true, false or a mapping with fars / bins (got {raw!r})")
    unknown = sorted(set(raw) - set(VERIFICATION_DEFAULTS))
    if unknown:
        raise ValueError(f"TRAIN.verification: unknown keys {unknown} (fars, bins)")
    out = dict(VERIFICATION_DEFAULTS, **raw)
    bins = out['bins']
    if isinstance(bins, bool) or not isinstance(bins, int) or not 2 <= bins <= 4096 or bins & (bins - 1):
        raise ValueError(f"TRAIN.verification: bins must be a power of two in [2, 4096] (got {bins!r})")
    fars = out['fars']
    if isinstance(fars, (int, float)) and not isinstance(fars, bool):
        fars = [fars]
    if not isinstance(fars, (list, tuple)) or not fars:
        raise ValueError(f"TRAIN.verification: fars must be a non-empty list (got {fars!r})")
    for f in fars:
        if isinstance(f, bool) or not isinstance(f, (int, float)) or not 0.0 < float(f) < 1.0:
            raise ValueError(f"TRAIN.verification: every far must lie in (0, 1) (got {f!r})")
    if not validate:
        raise ValueError("TRAIN.verification evaluates the validation set: it needs DATALOADER.validate (validation is off)")
    return {'fars': [float(f) for f in fars], 'bins': bins}


def verification_names(verification):
    """The history names (without 'val_') of a verification_config result, in logging order."""
    return ['auc', 'eer'] + [f'tar@far={f!r}' for f in verification['fars']] if verification else []


def monitored_value(monitor, history, epoch_loss):
    """What plateau, early stop and best checkpoint minimise: the monitored entry itself where lower is better (the losses,
    val_eer), 1 - it for every other evaluation value."""
    if monitor == 'loss':
        return epoch_loss
    last = history[monitor][-1]
    return last if monitor == 'val_loss' or monitor in LOWER_IS_BETTER else 1.0 - last


def monitor_config(p_train, validate):
    """TRAIN.retrieval_ks / TRAIN.monitor (both optional) -> (the K's of the per-epoch retrieval evaluation, the monitored name).
    retrieval_ks: after each epoch's validation, Recall@K and MRR of the validation set (leave-one-out,
    EmbeddingNet.calculate_retrieval_metrics) join the history as val_recall@K / val_mrr.  monitor: what plateau, early stop and
    best checkpoint follow — 'val_loss' ('loss' without validation) by default, or 'loss', 'val_recall@K' with K in
    retrieval_ks, 'val_mrr', with TRAIN.retrieval_map (retrieval_map_config) 'val_map@r' / 'val_r_precision', and with
    TRAIN.clustering_nmi (clustering_nmi_config) 'val_nmi' — larger is better for all of those —, and with TRAIN.verification
    (verification_config) 'val_auc', 'val_tar@far=f' (larger is better) or 'val_eer' (LOWER is better: monitored_value does not
    flip it).  Anything that cannot be honoured is a ValueError before training starts."""
    ks = p_train.get('retrieval_ks') or []
    if isinstance(ks, (int, float)):
        ks = [ks]
    if any(int(k) != k or int(k) < 1 for k in ks):
        raise ValueError(f"TRAIN.retrieval_ks: every K must be an integer >= 1 (got {list(ks)})")
    ks = [int(k) for k in ks]
    if ks and not validate:
        raise ValueError("TRAIN.retrieval_ks evaluates the validation set: it needs DATALOADER.validate (validation is off)")
    default = 'val_loss' if validate else 'loss'
    monitor = p_train.get('monitor') or default
    if monitor.startswith('val_') and not validate:
        raise ValueError(f"TRAIN.monitor: {monitor!r} needs DATALOADER.validate (validation is off)")
    if monitor.startswith('val_recall@'):
        if monitor not in [f'val_recall@{k}' for k in ks]:
            raise ValueError(f"TRAIN.monitor: {monitor!r} names a K that TRAIN.retrieval_ks {ks} does not compute")
    elif monitor == 'val_mrr':
        if not ks:
            raise ValueError("TRAIN.monitor: 'val_mrr' needs TRAIN.retrieval_ks")
    elif monitor in MAP_MONITORS:
        if not retrieval_map_config(p_train, validate):
            raise ValueError(f"TRAIN.monitor: {monitor!r} needs TRAIN.retrieval_map")
    elif monitor == 'val_nmi':
        if not clustering_nmi_config(p_train, validate):
            raise ValueError("TRAIN.monitor: 'val_nmi' needs TRAIN.clustering_nmi")
    elif monitor in ('val_auc', 'val_eer') or monitor.startswith('val_tar@far='):
        verification = verification_config(p_train, validate)
        if not verification:
            raise ValueError(f"TRAIN.monitor: {monitor!r} needs TRAIN.verification")
        if monitor[4:] not in verification_names(verification):
            raise ValueError(f"TRAIN.monitor: {monitor!r} names a far that TRAIN.verification.fars {verification['fars']} does not "
                             "compute")
    elif monitor not in ('loss', 'val_loss'):
        raise ValueError(f"TRAIN.monitor: unknown name {monitor!r} (loss, val_loss, val_recall@K, val_mrr, val_map@r, "
                         "val_r_precision, val_nmi, val_auc, val_eer, val_tar@far=f)")
    return ks, monitor


def main():
    args = parse_args()
    cfg = parse_params(args.config)
    device_augmentations(cfg, args.synthetic)          # a bad GENERATOR.device_augmentations fails before the GPU is touched
    monitor_config(cfg['train'], bool(cfg['dataloader'].get('validate', True)))      # likewise a bad TRAIN.monitor / retrieval_ks
    ms_loss = ms_loss_config(cfg)                      # likewise GENERATOR.ms_loss with another mode
    supcon_loss = supcon_loss_config(cfg)              # and GENERATOR.supcon_loss
    proxy_loss = proxy_loss_config(cfg)                # and GENERATOR.proxy_loss
    ap_loss = ap_loss_config(cfg)                      # and GENERATOR.ap_loss
    circle_loss = circle_loss_config(cfg)              # and GENERATOR.circle_loss
    margin_loss = margin_loss_config(cfg)              # and GENERATOR.margin_loss
    xbm = xbm_config(cfg)                              # and GENERATOR.xbm (with a proxy mode, in Siamese mode, a memory below a batch)
    # each is refused with another's mode: at most one is set
    loss_params = next((v for v in (ms_loss, supcon_loss, proxy_loss, ap_loss, circle_loss, margin_loss) if v is not None), None)
    multi_proxy_mode = cfg['generator'].get('negatives_selection_mode') in MULTI_PROXY_LOSS_CONFIGS
    proxy_mode = cfg['generator'].get('negatives_selection_mode') in PROXY_LOSS_KEYS or multi_proxy_mode
    # the modes whose log line carries the violating anchors: the ranking losses and Circle loss
    ap_mode = cfg['generator'].get('negatives_selection_mode') in tuple(AP_LOSS_KEYS) + ('circle',) and cfg['model']['mode'] != 'siamese'
    # the mode whose log line carries the active pairs per step: the margin loss's positive hinges
    margin_mode = cfg['generator'].get('negatives_selection_mode') == 'distance_weighted' and cfg['model']['mode'] != 'siamese'
    if proxy_mode and cfg['model']['mode'] == 'siamese':
        raise ValueError(f"negatives_selection_mode {cfg['generator']['negatives_selection_mode']!r} needs a triplet-mode model")
    retrieval_map_config(cfg['train'], bool(cfg['dataloader'].get('validate', True)))
    clustering_nmi_config(cfg['train'], bool(cfg['dataloader'].get('validate', True)))
    verification_config(cfg['train'], bool(cfg['dataloader'].get('validate', True)))
    p_train, p_model, p_loader, p_gen = cfg['train'], cfg['model'], cfg['dataloader'], cfg['generator']
    apply_gpu_ids(cfg['general'].get('gpu_ids'))
    paths = create_save_folders(cfg['general'])
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:        # before the first GPU call: stay on the cores next to this rank's GPU
        from embeddingnet_amd import launch
        print(f"[rank {os.environ.get('RANK', '0')}] {launch.pin_to_gpu_numa(int(os.environ.get('LOCAL_RANK', '0')))}", flush=True)
    rank, world, local = init_distributed()
    dev = torch.device('cuda', local % max(torch.cuda.device_count(), 1))    # (ranks > GPUs only in the gloo debug mode)
    torch.cuda.set_device(dev)
    p_model['device'] = dev
    # every rank builds the same dataset and the same initial model; what differs per rank is what it samples
    import random
    random.seed(1234 + rank)
    np.random.seed(1234 + rank)

    if args.synthetic:
        data_loader = SyntheticDataLoader(args.synthetic, 24, p_model['input_shape'],
                                          validate=p_loader.get('validate', True), seed=0)
    else:
        data_loader = ENDataLoader(**{k: v for k, v in p_loader.items() if k != 'csv_file'})
    retrieval_ks, monitor = monitor_config(p_train, bool(data_loader.validate))
    retrieval_map = retrieval_map_config(p_train, bool(data_loader.validate))
    clustering_nmi = clustering_nmi_config(p_train, bool(data_loader.validate))
    verification = verification_config(p_train, bool(data_loader.validate))
    gen_kw = {k: v for k, v in p_gen.items() if k not in ('device_augmentations', 'augment_seed', 'ms_loss', 'supcon_loss', 'proxy_loss',
                                                       'ap_loss', 'circle_loss', 'margin_loss', 'xbm')}

    siamese = p_model['mode'] == 'siamese'
    if siamese:
        model = SiameseNet(cfg, training=True)
        train_gen = SiameseDataGenerator(class_files_paths=data_loader.train_data, class_names=data_loader.class_names,
                                         **gen_kw)
        val_gen = SiameseDataGenerator(class_files_paths=data_loader.val_data, class_names=data_loader.class_names,
                                       val_gen=True, **gen_kw) if data_loader.validate else None
        trainable = model.model
    else:
        model = TripletNet(cfg, training=True)
        if world > 1:                                 # whole classes per rank, mining stays local
            _, gen_kw['k_classes'] = shard_classes(p_gen['k_classes'], world, rank)
        train_gen = TripletsDataGenerator(embedding_model=model.base_model, class_files_paths=data_loader.train_data,
                                          class_names=data_loader.class_names, **gen_kw,
                                          device_augmentations=device_augmentations(cfg, args.synthetic, rank))
        val_gen = SimpleTripletsDataGenerator(data_loader.val_data, data_loader.class_names,
                                              **gen_kw) if data_loader.validate else None
        trainable = model.base_model
    if args.resume_from is not None:
        model.load_model(args.resume_from)            # the mining model IS base_model, so it resumes too
    broadcast_model(trainable)                        # identical start on every rank: parameters and BN buffers
    head = None
    if proxy_mode:
        # one learnable proxy per class of the WHOLE dataset, replicated on every rank (seeded on the CPU: identical everywhere)
        from embeddingnet_amd.proxies import ProxyHead
        centers = 1
        if multi_proxy_mode:                          # ... or `centers` of them (the trainer checks the number against the head's)
            loss_params = dict(loss_params or {})
            centers = loss_params.setdefault('centers', MULTI_PROXY_DEFAULT_CENTERS[p_gen['negatives_selection_mode']])
        head = ProxyHead(len(data_loader.class_names), p_model['encodings_len'], seed=0, centers_per_class=centers).to(dev)
        if args.resume_from is not None and os.path.exists(_proxies_path(args.resume_from)):
            load_proxies(_proxies_path(args.resume_from), head, data_loader.class_names)
            print(f'resumed proxies from {_proxies_path(args.resume_from)}')
        broadcast_model(head)
    if 'softmax' in cfg:                              # reference train.py:164-170
        # every rank pre-trains on its own batches with the gradients all-reduced (no rank waits in a collective for the
        # length of a pre-training: the RCCL watchdog would abort it); rank 0 writes the pre-training checkpoints
        from embedding_net.backbones import pretrain_backbone_softmax
        pretrain_backbone_softmax(model.backbone_model, data_loader, cfg['softmax'], cfg['general'],
                                  max_epochs=args.max_epochs, distributed=world > 1)
        broadcast_model(trainable)                    # belt and braces: BN moving statistics are rank-local

    params = [p for p in trainable.parameters() if p.requires_grad] + ([head.proxies] if head is not None else [])

    def named_slots():
        """The parameters whose optimizer slots a checkpoint holds, by name: the Keras weight names, and the proxies."""
        from embeddingnet_amd.backbones import keras_weights
        named = {k: v for k, v in keras_weights(trainable).items() if isinstance(v, torch.nn.Parameter)}
        if head is not None:
            named['proxy_head/proxies'] = head.proxies
        return named

    # TRAIN.optimizer_params (utils.OptimizerSpec.build): groups 'kernels' / 'other' / 'proxies' with their decay and rate multiplier;
    # without the key this is the reference's optimizer over `params`, the proxies one more tensor of its single group
    opt = p_train['optimizer'].build(params[:len(params) - (head is not None)], proxies=[head.proxies] if head is not None else None)
    clipnorm = bool(getattr(opt, 'global_clipnorm', 0))
    # optimizers 'lars' / 'lamb': the tensors whose steps are adapted (every group but 'other'), for the epoch line's trust ratios
    adapted = torch.tensor(opt.adapted, dtype=torch.long, device=dev) if getattr(opt, 'layerwise', False) else None
    lr0 =p_train['learning_rate']
    resumed_updates = 0
    if args.resume_from is not None:                  # optimizer slots and step count, when the checkpoint has them (Keras'
        # load_model restores the optimizer with the weights; the epoch count and LR schedule restart, as in the reference)
        from embeddingnet_amd.optimizers import load_optimizer_state
        opt_path = _optimizer_state_path(args.resume_from)
        if os.path.exists(opt_path):
            extra = load_optimizer_state(opt_path, opt, named_slots())
            print(f'resumed optimizer state from {opt_path} (iterations {opt.iterations}, saved after epoch {int(extra.get("epoch", 0))})')
            resumed_updates = int(extra.get('n_averaged', 0))
    averager, averaging = None, p_train.get('weight_averaging')
    if averaging is not None:
        # the averages start as copies of the model as it is now (initial, or resumed): the base model's tensors, BatchNorm moving
        # statistics included, and the proxies.  Parameters' averages stay bitwise equal across data-parallel ranks (the same
        # coefficient, the same weights); buffers' are rank-local and are averaged over the ranks when a checkpoint is written
        averager = build_averager(averaging, [trainable] + ([head] if head is not None else []), len(train_gen))
        if args.resume_from is not None:
            avg_path = _averaged_path(args.resume_from)
            if os.path.exists(avg_path):
                with np.load(avg_path, allow_pickle=False) as d:
                    averager.load_averaged({k: d[k] for k in d.files})          # other names or shapes are refused
                averager.set_counters((opt.iterations, resumed_updates))
                print(f'resumed averaged weights from {avg_path} (averaged {averager.n_averaged})')
            else:
                averager.set_counters((opt.iterations, 0))
                print(f'no averaged weights at {avg_path}: the averages start from the resumed model')

    def evaluation():
        """What validation runs inside: the averages in the model once there are any (evaluate 'averaged'), else nothing."""
        import contextlib
        if averager is not None and averaging['evaluate'] == 'averaged' and averager.n_averaged > 0:
            return averager.applied()
        return contextlib.nullcontext()
    reducer = GradReducer(params) if world > 1 else None
    if siamese:
        # the Siamese step (reference train.py:108-119: fit of SiameseNet.model with contrastive_loss) as a trainer: its own step
        # context, one-launch optimizer, and a captured step where the host cannot keep up (EMBNET_GRAPH=auto)
        from embeddingnet_amd.train_step import SiameseTrainer
        trainer = SiameseTrainer(model.model, opt, contrastive_loss, seed=rank, reducer=reducer, averager=averager)
    elif proxy_mode:
        # each rank's loss covers its own batch against ALL proxies; the reducer's mean over the ranks' gradients is the gradient
        # of the mean of the ranks' losses, for the (replicated) proxies as for the backbone (train_step.ProxyTrainer)
        from embeddingnet_amd.train_step import ProxyTrainer
        trainer = ProxyTrainer(model.base_model, head, opt, loss=p_gen['negatives_selection_mode'], loss_params=loss_params,
                               seed=rank, reducer=reducer, averager=averager)
    else:
        kw = dict(margin=p_gen['margin'], negatives_selection_mode=p_gen['negatives_selection_mode'], seed=rank, reducer=reducer,
                  loss_params=loss_params, averager=averager)
        if xbm is not None:
            # each rank keeps a memory of its own batches (nothing is gathered); it starts empty, after a resume too
            from embeddingnet_amd.train_step import XbmTrainer
            from embeddingnet_amd.xbm import CrossBatchMemory
            memory = CrossBatchMemory(xbm['size'], p_model['encodings_len'], dev)
            trainer = XbmTrainer(model.base_model, opt, gen_kw['k_classes'], p_gen['k_samples'], memory=memory, xbm_loss=xbm['loss'],
                                 xbm_params=xbm['params'], weight=xbm['weight'], start_iteration=xbm['start_iteration'], **kw)
        else:
            trainer = TripletTrainer(model.base_model, opt, gen_kw['k_classes'], p_gen['k_samples'], **kw)
    plateau = Plateau(persistent=bool(p_train.get('plateau_persistent', False)))
    history = {'loss': [], 'val_loss': []}
    for k in retrieval_ks:
        history[f'val_recall@{k}'] = []
    if retrieval_ks:
        history['val_mrr'] = []
    if retrieval_map:
        history['val_map@r'], history['val_r_precision'] = [], []
    if clustering_nmi:
        history['val_nmi'] = []
    for name in verification_names(verification):
        history['val_' + name] = []
    n_epochs = min(p_train['n_epochs'], args.max_epochs or p_train['n_epochs'])
    from embeddingnet_amd.layers import GeM
    gem_layers = [m for m in trainable.modules() if isinstance(m, GeM)]     # MODEL.pooling 'gem': the exponent is logged per epoch

    # triplet mode: batches are planned on this thread and decoded / uploaded ahead of the step (input_pipeline.Feeder: the
    # role of Keras' fit_generator enqueuer, reference train.py:172-177)
    feeder = None if siamese else train_gen.feeder(dev, log=(print if rank == 0 else None))
    import time
    try:        # (the feeder owns worker processes and a staging file in /dev/shm: released on ANY exit)
        for epoch in range(n_epochs):
            t_epoch, n_images = time.perf_counter(), 0
            # LearningRateScheduler.on_epoch_begin (reference train.py:80-81): sets the rate outright, which discards the
            # previous epoch's ReduceLROnPlateau reduction (see Plateau) unless TRAIN.plateau_persistent is set
            lr = lr0 * p_train['decay_factor'] ** np.floor(epoch / p_train['step_size'])
            if plateau.persistent:
                lr *= plateau.scale
            for g in opt.param_groups:
                g['lr'] = lr
            trainable.train()
            losses, xbm_counts, violating, active_pairs = [], [], [], []
            norm_sum = torch.zeros((), dtype=torch.float64, device=dev) if clipnorm else None     # summed on the device, read once per epoch
            for _ in range(len(train_gen)):
                if norm_sum is not None and losses:
                    norm_sum += opt.grad_norm             # the step before's norm before clipping (the last one joins behind the loop)
                if siamese:
                    (x1, x2), y = train_gen[0]
                    losses.append(trainer.step(torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev),
                                               torch.from_numpy(np.asarray(y, dtype=np.float32)).to(dev).reshape(-1, 1)))
                else:
                    if proxy_mode or xbm is not None:
                        xb, yb = feeder.next_labelled()
                        losses.append(trainer.step(xb, yb))
                        if multi_proxy_mode or ap_mode:
                            violating.append(trainer.last_triplets[1].clone())      # (a replayed step's counts are one buffer)
                        if margin_mode:
                            active_pairs.append(trainer.last_triplets[1].clone())
                        if xbm is not None and trainer.last_xbm_counts is not None:
                            xbm_counts.append(trainer.last_xbm_counts.clone())      # (a replayed step's counts are one buffer)
                    else:
                        xb = feeder.next()
                        losses.append(trainer.step(xb))
                        if ap_mode:                       # the violating anchors (a replayed step's counts are one buffer)
                            violating.append(trainer.last_triplets[1].clone())
                        if margin_mode:                   # the positive hinges, likewise
                            active_pairs.append(trainer.last_triplets[1].clone())
                    n_images += xb.shape[0]
            epoch_loss = all_reduce_mean(float(torch.stack(losses).mean().item()))     # mean over ranks (logging + monitor)
            history['loss'].append(epoch_loss)
            msg = f'Epoch {epoch + 1}/{n_epochs} - lr {lr:.3g} - loss {epoch_loss:.4f}'
            if n_images:                                  # (the .item() above waited for the epoch's last step)
                msg += f' - {n_images * world / (time.perf_counter() - t_epoch):.0f} images/s'
            if violating:                                 # this rank's: violating samples (anchors) per step, the last step's regulariser
                msg += f' - violating {torch.stack(violating).float().mean().item():.1f}'
                if multi_proxy_mode and trainer.last_reg is not None:
                    msg += f' - reg {trainer.last_reg.item():.4f}'
            if active_pairs:                              # this rank's: hinges above zero per step, positives' and drawn negatives'
                msg += f' - active_pairs {torch.stack(active_pairs).float().mean().item():.1f}'
            if norm_sum is not None and losses:           # this rank's: the mean global gradient norm before clipping
                norm_sum += opt.grad_norm
                msg += f' - grad_norm {norm_sum.item() / len(losses):.4g}'
            if adapted is not None and adapted.numel() and losses:      # this rank's: the last step's trust ratios, smallest..largest
                ratios = opt.trust_ratios[adapted]
                msg += f' - trust {ratios.min().item():.3g}..{ratios.max().item():.3g}'
            if xbm is not None:                           # this rank's memory: labelled slots now, pairs kept over the epoch
                kept = torch.stack(xbm_counts).sum(0).tolist() if xbm_counts else [0, 0]
                msg += f' - xbm_filled {memory.filled()} - xbm_kept {kept[0]}+{kept[1]}'
            if averager is not None:
                msg += f' - averaged {averager.n_averaged}'
            if gem_layers:                                # the live exponent (the mean of a per-channel one), read once per epoch
                msg += f' - gem_p {torch.cat([m.p.detach().reshape(-1) for m in gem_layers]).mean().item():.4f}'
            value = epoch_loss
            if val_gen is not None:
                with evaluation():                    # (TRAIN.weight_averaging: the averaged weights, planes and ranges)
                    trainable.eval()
                    vals = []
                    with torch.no_grad():
                        for _ in range(len(val_gen)):
                            xs, y = val_gen[0]
                            xs = [torch.from_numpy(a).to(dev) for a in xs]
                            if siamese:
                                out = model.model(xs)[0]
                                vals.append(contrastive_loss(torch.from_numpy(y).to(dev), out))
                            else:
                                vals.append(triplet_loss(p_gen['margin'])(None, model.model(xs)).mean())
                    value = all_reduce_mean(float(torch.stack(vals).mean().item()))
                    history['val_loss'].append(value)
                    msg += f' - val_loss {value:.4f}'
                    if retrieval_ks:
                        # every rank evaluates the whole validation set (BN buffers are rank-local, decisions must agree): the
                        # values pass through all_reduce_mean like val_loss
                        with torch.no_grad():
                            found = model.calculate_retrieval_metrics(data_loader, ks=retrieval_ks)
                        for name in [f'recall@{k}' for k in retrieval_ks] + ['mrr']:
                            history['val_' + name].append(all_reduce_mean(float(found[name])))
                            msg += f" - val_{name} {history['val_' + name][-1]:.4f}"
                    if retrieval_map:
                        with torch.no_grad():
                            found = model.calculate_map_at_r(data_loader)
                        for name in ('map@r', 'r_precision'):
                            history['val_' + name].append(all_reduce_mean(float(found[name])))
                            msg += f" - val_{name} {history['val_' + name][-1]:.4f}"
                    if clustering_nmi:
                        with torch.no_grad():
                            found = model.calculate_clustering_metrics(data_loader)
                        history['val_nmi'].append(all_reduce_mean(float(found['nmi'])))
                        msg += f" - val_nmi {history['val_nmi'][-1]:.4f}"
                    if verification:
                        with torch.no_grad():
                            found = model.calculate_verification_metrics(data_loader, fars=verification['fars'],
                                                                         bins=verification['bins'])
                        for name in verification_names(verification):
                            history['val_' + name].append(all_reduce_mean(float(found[name])))
                            msg += f" - val_{name} {history['val_' + name][-1]:.4f}"
                    value = monitored_value(monitor, history, epoch_loss)    # lower is better for plateau, early stop, best checkpoint
            if rank == 0:
                print(msg, flush=True)
            improved, stop, lr_end = plateau.update(value, lr)   # `value` is the all-reduced mean: same decisions on every rank
            for g in opt.param_groups:                    # ReduceLROnPlateau.on_epoch_end (until the scheduler's next epoch begin)
                g['lr'] = lr_end
            if improved:
                average_buffers(trainable)                # BN moving statistics: mean over the ranks' local batches
                if averager is not None:
                    averager.average_buffers()            # ... and their averages, which are rank-local too
            if improved and rank == 0:
                path = os.path.join(paths['weights'], f'epoch_{epoch + 1:03d}.npz')
                model.save_weights(path)
                from embeddingnet_amd.optimizers import save_optimizer_state
                os.makedirs(os.path.dirname(_optimizer_state_path(path)), exist_ok=True)
                extra = {'epoch': epoch + 1}
                if averager is not None:
                    extra['n_averaged'] = averager.n_averaged
                    os.makedirs(os.path.dirname(_averaged_path(path)), exist_ok=True)
                    np.savez(_averaged_path(path), **{k: v.detach().cpu().numpy() for k, v in averager.averaged.items()})
                save_optimizer_state(_optimizer_state_path(path), opt, named_slots(), extra=extra)
                if head is not None:
                    save_proxies(_proxies_path(path), head, data_loader.class_names)
                print(f'{monitor} improved to {history[monitor][-1]:.5f}, saving model to {path}')
            if stop:
                print('EarlyStopping')
                break
    finally:
        if feeder is not None:
            feeder.close()                            # decode worker processes, staging file in /dev/shm
    if rank == 0:
        np.savez(os.path.join(paths['plots'], 'history.npz'), **{k: np.asarray(v) for k, v in history.items()})
    dump = os.environ.get('EMBNET_DUMP_FINAL_WEIGHTS')     # diagnostics: EVERY rank's final weights -> <prefix><rank>.npz
    if dump:                                               # (data-parallel ranks must end with identical trainable weights)
        model.save_weights(f'{dump}{rank}.npz')
        if head is not None:
            save_proxies(f'{dump}{rank}_proxies.npz', head, data_loader.class_names)
    return history


if __name__ == '__main__':
    main()
