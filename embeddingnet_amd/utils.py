"""Drop-in for the config / optimizer part of embedding_net/utils.py (reference :143-197) and for its encodings plots
(`load_encodings`, `plot_tsne`, `plot_tsne_interactive`, reference :29-91; the t-SNE itself is embeddingnet_amd/tsne.py,
exact and on the device, where the reference calls scikit-learn).

`parse_params` keeps the reference's YAML schema and the layout of the dict it returns (lower-case
section keys; MODEL.input_shape mirrored into GENERATOR and SOFTMAX_PRETRAINING; the optimizer entry of a
section replaced by an optimizer object; `augmentations` keys set).  One structural difference: Keras
optimizers are constructed without parameters, ours need them, so the optimizer object is an
`OptimizerSpec` whose `.build(parameters)` returns the optimizer (embeddingnet_amd/optimizers.py: the
Keras update rules and defaults, one HIP launch per step).  GENERATOR keys pass through as written, among them
`device_augmentations` / `augment_seed` (tools/train.py: on-device augmentation, embeddingnet_amd/augment.py).
"""
import os
import pickle
import sys

import yaml

# YAML section -> key of the returned dict (reference utils.py:169-195); the last one is optional
SECTIONS = (("DATALOADER", "dataloader"), ("GENERATOR", "generator"), ("MODEL", "model"), ("TRAIN", "train"),
            ("GENERAL", "general"), ("ENCODINGS", "encodings"))
OPTIONAL_SECTION = ("SOFTMAX_PRETRAINING", "softmax")


class OptimizerSpec:
    """What `get_optimizer(name, lr)` returns: the optimizer's rule and learning rate, bound to parameters later."""

    def __init__(self, name, learning_rate, params=None):
        self.name, self.learning_rate = name, float(learning_rate)
        self.params = check_optimizer_params(params)

    @property
    def rule(self):
        """reference utils.py:144-152: 'adam', 'rms_prop', 'radam', anything else is plain SGD — and, beyond the reference, the
        layer-wise adaptive 'lars' and 'lamb'."""
        return self.name if self.name in ("adam", "rms_prop", "radam") + LAYERWISE_RULES else "sgd"

    def build(self, parameters, proxies=None):
        """parameters: the model's.  Without `optimizer_params` the reference's optimizer over one group (`proxies`, when a
        proxy mode has them, are one more tensor of it).  With them up to three groups: 'kernels' — parameters with two or more
        dimensions, which get `weight_decay` — 'other' — BatchNorm parameters and biases, never decayed — and 'proxies' with
        `proxy_lr_mult` and `proxy_weight_decay`; `group_names` on the optimizer lists the groups built.
        'lars' and 'lamb' always get these groups, with or without `optimizer_params`: 'other' is neither decayed nor adapted
        (trust coefficient 0: the exclusion of BatchNorm parameters and biases in SimCLR's and LAMB's recipes, which also covers a
        GeM exponent), 'kernels' and 'proxies' are adapted with `trust_coefficient` (default: the rule's)."""
        from .optimizers import KerasOptimizer
        parameters = list(parameters)
        proxies = list(proxies or [])
        layerwise = self.rule in LAYERWISE_RULES
        o = self.params
        if "trust_coefficient" in o and not layerwise:
            raise ValueError(f"optimizer_params: trust_coefficient belongs to the optimizers 'lars' and 'lamb', not {self.name!r}")
        if not o and not layerwise:
            return KerasOptimizer(parameters + proxies, self.rule, self.learning_rate)
        if not proxies and ("proxy_lr_mult" in o or "proxy_weight_decay" in o):
            raise ValueError("optimizer_params: proxy_lr_mult / proxy_weight_decay belong to the proxy modes")
        groups = [("kernels", dict(params=[p for p in parameters if p.dim() >= 2], weight_decay=float(o.get("weight_decay", 0.0)))),
                  ("other", dict(params=[p for p in parameters if p.dim() < 2], **(dict(trust_coefficient=0.0) if layerwise else {}))),
                  ("proxies", dict(params=proxies, lr_mult=float(o.get("proxy_lr_mult", 1.0)),
                                   weight_decay=float(o.get("proxy_weight_decay", 0.0))))]
        groups = [(n, g) for n, g in groups if g["params"]]
        kwargs = {k: o[k] for k in ("momentum", "nesterov", "epsilon", "beta_1", "beta_2", "clipvalue", "global_clipnorm",
                                    "trust_coefficient") if k in o}
        opt = KerasOptimizer([g for _, g in groups], self.rule, self.learning_rate, **kwargs)
        opt.group_names = [n for n, _ in groups]
        return opt

    def __repr__(self):
        extra = f", params={self.params}" if self.params else ""
        return f"OptimizerSpec({self.name!r}, lr={self.learning_rate}{extra})"


OPTIMIZER_PARAMS = ("weight_decay", "momentum", "nesterov", "epsilon", "beta_1", "beta_2", "clipvalue", "global_clipnorm",
                    "proxy_lr_mult", "proxy_weight_decay", "trust_coefficient")
LAYERWISE_RULES = ("lars", "lamb")


def check_optimizer_params(params):
    """TRAIN.optimizer_params -> a dict with known keys only (unknown ones are refused; so is a `trust_coefficient` that is not a
    number >= 0)."""
    params = dict(params or {})
    unknown = set(params) - set(OPTIMIZER_PARAMS)
    if unknown:
        raise ValueError(f"optimizer_params: unknown keys {sorted(unknown)} ({', '.join(OPTIMIZER_PARAMS)})")
    eta = params.get("trust_coefficient", 0.0)
    if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not eta >= 0:
        raise ValueError(f"optimizer_params: trust_coefficient must be a number >= 0 (got {eta!r})")
    return params


def get_optimizer(name, learning_rate, params=None):
    return OptimizerSpec(name, learning_rate, params)


WEIGHT_AVERAGING_KEYS = ("mode", "decay", "warmup", "start_epoch", "update_every", "evaluate")


def check_weight_averaging(section):
    """TRAIN.weight_averaging -> a dict with every key filled in (weight_average.WeightAverager's arguments, in epochs where the
    trainer counts steps); unknown keys, wrong types and values outside their range are refused.
      mode          'ema' | 'swa'
      decay         ema only, inside (0, 1), default 0.999;   warmup: ema only, a boolean, default true
      start_epoch   default 0: the averaging starts after that many epochs
      update_every  a step count >= 1, or 'epoch' (one update per epoch); default 1 for ema, 'epoch' for swa
      evaluate      'averaged' (default): validation, monitor and the final encodings use the averages;  'model': the live weights"""
    if not isinstance(section, dict):
        raise ValueError("weight_averaging: a mapping of " + ", ".join(WEIGHT_AVERAGING_KEYS))
    unknown = set(section) - set(WEIGHT_AVERAGING_KEYS)
    if unknown:
        raise ValueError(f"weight_averaging: unknown keys {sorted(unknown)} ({', '.join(WEIGHT_AVERAGING_KEYS)})")
    mode = section.get("mode")
    if mode not in ("ema", "swa"):
        raise ValueError(f"weight_averaging: mode must be 'ema' or 'swa' (got {mode!r})")
    out = dict(mode=mode)
    if mode == "swa":
        for key in ("decay", "warmup"):
            if key in section:
                raise ValueError(f"weight_averaging: {key} belongs to mode 'ema', not 'swa'")
    else:
        decay, warmup = section.get("decay", 0.999), section.get("warmup", True)
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < decay < 1.0:
            raise ValueError(f"weight_averaging: decay must be a number inside (0, 1) (got {decay!r})")
        if not isinstance(warmup, bool):
            raise ValueError(f"weight_averaging: warmup must be true or false (got {warmup!r})")
        out.update(decay=float(decay), warmup=warmup)
    start = section.get("start_epoch", 0)
    if isinstance(start, bool) or not isinstance(start, int) or start < 0:
        raise ValueError(f"weight_averaging: start_epoch must be a whole number >= 0 (got {start!r})")
    every = section.get("update_every", 1 if mode == "ema" else "epoch")
    if every != "epoch" and (isinstance(every, bool) or not isinstance(every, int) or every < 1):
        raise ValueError(f"weight_averaging: update_every must be a step count >= 1 or 'epoch' (got {every!r})")
    evaluate = section.get("evaluate", "averaged")
    if evaluate not in ("averaged", "model"):
        raise ValueError(f"weight_averaging: evaluate must be 'averaged' or 'model' (got {evaluate!r})")
    out.update(start_epoch=start, update_every=every, evaluate=evaluate)
    return out


POOLING_TYPES = ("avg", "gem")
POOLING_KEYS = ("type", "p", "eps", "learnable", "per_channel")


def check_pooling(pooling, backbone_name=None):
    """MODEL.pooling -> None for the average-pooling head (None, 'avg', {'type': 'avg'}), or for GeM ('gem' or a mapping with
    type 'gem') a dict with every key of layers.GeM filled in: p (3.0), eps (1e-6), learnable (true), per_channel (false).
    Unknown types, unknown keys and wrong value types are refused by key; so is anything but 'avg' for the backbones whose
    heads do not pool ('simple', 'simple2')."""
    if pooling is None or isinstance(pooling, str):
        pooling = {"type": pooling or "avg"}
    if not isinstance(pooling, dict):
        raise ValueError(f"pooling: a type name ({', '.join(POOLING_TYPES)}) or a mapping of {', '.join(POOLING_KEYS)} "
                         f"(got {pooling!r})")
    unknown = set(pooling) - set(POOLING_KEYS)
    if unknown:
        raise ValueError(f"pooling: unknown keys {sorted(unknown, key=str)} ({', '.join(POOLING_KEYS)})")
    kind = pooling.get("type")
    if kind not in POOLING_TYPES:
        raise ValueError(f"pooling: type must be one of {', '.join(POOLING_TYPES)} (got {kind!r})")
    if kind == "avg":
        if len(pooling) > 1:
            raise ValueError(f"pooling: {sorted(set(pooling) - {'type'})} belong to type 'gem', not 'avg'")
        return None
    if backbone_name in ("simple", "simple2"):
        raise ValueError(f"pooling: type 'gem' needs a pooling head; the head of backbone '{backbone_name}' does not pool")
    out = dict(type="gem")
    for key, default in (("p", 3.0), ("eps", 1e-6)):
        v = pooling.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
            raise ValueError(f"pooling: {key} must be a number > 0 (got {v!r})")
        out[key] = float(v)
    for key, default in (("learnable", True), ("per_channel", False)):
        v = pooling.get(key, default)
        if not isinstance(v, bool):
            raise ValueError(f"pooling: {key} must be true or false (got {v!r})")
        out[key] = v
    return out


def _finish_section(section, input_shape):
    """A section that drives training (TRAIN-like or SOFTMAX_PRETRAINING): optimizer name -> object."""
    section['optimizer'] = get_optimizer(section['optimizer'], section['learning_rate'], section.get('optimizer_params'))
    if 'weight_averaging' in section:
        section['weight_averaging'] = check_weight_averaging(section['weight_averaging'])
    if input_shape is not None:
        section['input_shape'] = input_shape
        # The reference builds albumentations pipelines only under the misspelt key 'augmentations_type'
        # (utils.py:160-164), i.e. never with the shipped configs; image augmentation is outside the hot path.
        section['augmentations'] = None
    return section


def parse_params(filename='configs/road_signs.yml'):
    with open(filename, 'r') as ymlfile:
        cfg = yaml.safe_load(ymlfile)
    params = {key: (cfg[section] if section != "ENCODINGS" else cfg.get(section, {})) for section, key in SECTIONS}
    shape = params['model']['input_shape']
    if 'pooling' in params['model']:                       # refused here, before anything is loaded or built
        check_pooling(params['model']['pooling'], params['model'].get('backbone_name', 'simple'))
    params['generator']['input_shape'] = shape
    params['generator']['augmentations'] = None
    _finish_section(params['train'], None)
    section, key = OPTIONAL_SECTION
    if section in cfg:
        params[key] = _finish_section(cfg[section], shape)
    return params


# --------------------------------------------------------------------------- encodings plots (reference utils.py:29-91)
def load_encodings(path_to_encodings):
    """The dict EmbeddingNet.save_encodings pickled: {'encodings': [n,e], 'labels': [n]}."""
    with open(path_to_encodings, 'rb') as f:
        return pickle.load(f)


def _has_display():
    if sys.platform.startswith(("win", "darwin")):
        return True
    return bool(os.environ.get("DISPLAY") or os.environ.get("WAYLAND_DISPLAY"))


def _tsne_by_label(encodings):
    """-> (embedding [n,2], [(label, xs, ys)] in list(set(labels)) order, as the reference iterates)."""
    import numpy as np
    from .tsne import TSNE
    emb = TSNE().fit_transform(np.asarray(encodings['encodings'], dtype=np.float32))
    names = np.array(encodings['labels'])
    return emb, [(l, emb[names == l, 0], emb[names == l, 1]) for l in list(set(encodings['labels']))]


def plot_tsne(encodings_path, save_plot_dir, show=True):
    """t-SNE scatter of saved encodings: one series per label, the label written above every point, legend outside the axes,
    16 x 16 inches, saved as `save_plot_dir + 'tsne.png.png'` (the reference's file name).  Without a display the Agg
    backend is used and `show` does nothing.  Returns the [n,2] embedding (the reference returns None)."""
    import matplotlib
    headless = not _has_display()
    if headless:
        matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    emb, series = _tsne_by_label(load_encodings(encodings_path))
    fig, ax = plt.subplots(figsize=(16, 16))
    for label, xs, ys in series:
        ax.scatter(xs, ys, label=label)
        for x, y in zip(xs, ys):
            ax.annotate(label, (x, y), size=8, textcoords="offset points", xytext=(0, 10), ha='center')
    ax.legend(bbox_to_anchor=(1.05, 1), fontsize='small', ncol=2)
    if show and not headless:
        fig.show()
    fig.savefig("{}{}.png".format(save_plot_dir, 'tsne.png'))
    plt.close(fig)
    return emb


def plot_tsne_interactive(encodings):
    """The same embedding as a plotly figure (markers named by label, 1000 x 1000); `encodings` is the dict or its path.
    Returns the [n,2] embedding."""
    try:
        import plotly.graph_objects as go
    except ImportError as err:
        raise ImportError("plot_tsne_interactive needs the 'plotly' package, which is not installed") from err
    import numpy as np
    if isinstance(encodings, str):
        encodings = load_encodings(encodings)
    emb, series = _tsne_by_label(encodings)
    fig = go.Figure()
    for label, xs, ys in series:
        r, g, b = (int(255 * np.random.rand()) for _ in range(3))
        fig.add_trace(go.Scatter(x=xs, y=ys, mode='markers', marker=dict(color=f'rgba({r},{g},{b},0.8)', size=10),
                                 text=str(label), name=str(label)))
    fig.update_layout(title=go.layout.Title(text="t-SNE plot", xref="paper", x=0), autosize=False, width=1000, height=1000)
    if _has_display():
        fig.show()
    return emb
