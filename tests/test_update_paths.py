"""CPU: which update path ``compile()`` derives for the tables and for the dense parameters, over optimizer classes,
hyper-parameters that rule a path out (weight_decay, momentum, nesterov, maximize, lr_decay, amsgrad, centered), parameter
group layouts and table regularisation.  The expected values were recorded from the three hand-written selectors
(``_sparse_update_mode`` / ``_lazy_update_mode`` / ``_dense_update_mode``) before they were folded into
``_hip/update_paths.match_optimizer``; they are literals, not recomputed here."""
import pytest
import torch

from helpers import build_model, load_golden

O = torch.optim
CONFIGS = {
    "sgd": (O.SGD, dict(lr=0.05)),
    "sgd-momentum": (O.SGD, dict(lr=0.05, momentum=0.9)),
    "sgd-wd": (O.SGD, dict(lr=0.05, weight_decay=1e-4)),
    "sgd-nesterov": (O.SGD, dict(lr=0.05, momentum=0.9, nesterov=True)),
    "sgd-maximize": (O.SGD, dict(lr=0.05, maximize=True)),
    "adagrad": (O.Adagrad, dict(lr=0.02)),
    "adagrad-lrdecay": (O.Adagrad, dict(lr=0.02, lr_decay=0.1)),
    "adagrad-wd": (O.Adagrad, dict(lr=0.02, weight_decay=1e-4)),
    "adagrad-maximize": (O.Adagrad, dict(lr=0.02, maximize=True)),
    "adagrad-eps": (O.Adagrad, dict(lr=0.02, eps=1e-8)),
    "adam": (O.Adam, dict(lr=0.002)),
    "adam-amsgrad": (O.Adam, dict(lr=0.002, amsgrad=True)),
    "adam-wd": (O.Adam, dict(lr=0.002, weight_decay=1e-4)),
    "adam-maximize": (O.Adam, dict(lr=0.002, maximize=True)),
    "adam-betas": (O.Adam, dict(lr=0.002, betas=(0.8, 0.99))),
    "rmsprop": (O.RMSprop, dict(lr=0.003)),
    "rmsprop-momentum": (O.RMSprop, dict(lr=0.003, momentum=0.9)),
    "rmsprop-centered": (O.RMSprop, dict(lr=0.003, centered=True)),
    "rmsprop-alpha": (O.RMSprop, dict(lr=0.003, alpha=0.9)),
    "rmsprop-wd": (O.RMSprop, dict(lr=0.003, weight_decay=1e-4)),
    "adamw": (O.AdamW, dict(lr=0.002)),
}
LAYOUTS = ("one", "two-equal", "two-lr", "table-missing")
L2S = (0.0, 1e-5)

# (plan.update, (lazy.kind, lazy.hyper) | None, dense mode, parameters that own optimizer state after compile(), its keys)
# per (configuration, layout, l2 of the tables).  State owners: "optimizer" = every parameter the optimizer holds (Adagrad
# creates its state at construction), "tables" = the plan's tables (seeded for the lazy replay), "none".
DENSE = ("dense",)
AG_KEYS, ADAM_KEYS, RMS_KEYS = ("step", "sum"), ("exp_avg", "exp_avg_sq", "step"), ("square_avg", "step")
EXPECTED = {
    ('sgd', 'one', 0.0): (('sgd', 0.05), None, ('sgd', 0.05), 'none', ()),
    ('sgd', 'one', 1e-05): (('lazy', 'sgd'), ('sgd', (0.05, 0.0, 0.0, 0.0)), ('sgd', 0.05), 'none', ()),
    ('sgd', 'two-equal', 0.0): (('sgd', 0.05), None, ('sgd', 0.05), 'none', ()),
    ('sgd', 'two-equal', 1e-05): (('lazy', 'sgd'), ('sgd', (0.05, 0.0, 0.0, 0.0)), ('sgd', 0.05), 'none', ()),
    ('sgd', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd', 'table-missing', 0.0): (DENSE, None, ('sgd', 0.05), 'none', ()),
    ('sgd', 'table-missing', 1e-05): (DENSE, None, ('sgd', 0.05), 'none', ()),
    ('sgd-momentum', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-momentum', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-momentum', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-momentum', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-momentum', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-momentum', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-momentum', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-momentum', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-wd', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-nesterov', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('sgd-maximize', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('adagrad', 'one', 0.0): (('adagrad', 0.02, 1e-10), None, ('adagrad', 0.02, 1e-10), 'optimizer', AG_KEYS),
    ('adagrad', 'one', 1e-05): (('lazy', 'adagrad'), ('adagrad', (0.02, 1e-10, 0.0, 0.0)), ('adagrad', 0.02, 1e-10), 'optimizer', AG_KEYS),
    ('adagrad', 'two-equal', 0.0): (('adagrad', 0.02, 1e-10), None, ('adagrad', 0.02, 1e-10), 'optimizer', AG_KEYS),
    ('adagrad', 'two-equal', 1e-05): (('lazy', 'adagrad'), ('adagrad', (0.02, 1e-10, 0.0, 0.0)), ('adagrad', 0.02, 1e-10), 'optimizer', AG_KEYS),
    ('adagrad', 'two-lr', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad', 'two-lr', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad', 'table-missing', 0.0): (DENSE, None, ('adagrad', 0.02, 1e-10), 'optimizer', AG_KEYS),
    ('adagrad', 'table-missing', 1e-05): (DENSE, None, ('adagrad', 0.02, 1e-10), 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'one', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'one', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'two-equal', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'two-equal', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'two-lr', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'two-lr', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'table-missing', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-lrdecay', 'table-missing', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'one', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'one', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'two-equal', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'two-equal', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'two-lr', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'two-lr', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'table-missing', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-wd', 'table-missing', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'one', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'one', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'two-equal', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'two-equal', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'two-lr', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'two-lr', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'table-missing', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-maximize', 'table-missing', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-eps', 'one', 0.0): (('adagrad', 0.02, 1e-08), None, ('adagrad', 0.02, 1e-08), 'optimizer', AG_KEYS),
    ('adagrad-eps', 'one', 1e-05): (('lazy', 'adagrad'), ('adagrad', (0.02, 1e-08, 0.0, 0.0)), ('adagrad', 0.02, 1e-08), 'optimizer', AG_KEYS),
    ('adagrad-eps', 'two-equal', 0.0): (('adagrad', 0.02, 1e-08), None, ('adagrad', 0.02, 1e-08), 'optimizer', AG_KEYS),
    ('adagrad-eps', 'two-equal', 1e-05): (('lazy', 'adagrad'), ('adagrad', (0.02, 1e-08, 0.0, 0.0)), ('adagrad', 0.02, 1e-08), 'optimizer', AG_KEYS),
    ('adagrad-eps', 'two-lr', 0.0): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-eps', 'two-lr', 1e-05): (DENSE, None, None, 'optimizer', AG_KEYS),
    ('adagrad-eps', 'table-missing', 0.0): (DENSE, None, ('adagrad', 0.02, 1e-08), 'optimizer', AG_KEYS),
    ('adagrad-eps', 'table-missing', 1e-05): (DENSE, None, ('adagrad', 0.02, 1e-08), 'optimizer', AG_KEYS),
    ('adam', 'one', 0.0): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.9, 0.999)), ('adam', 0.002, 1e-08, 0.9, 0.999), 'tables', ADAM_KEYS),
    ('adam', 'one', 1e-05): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.9, 0.999)), ('adam', 0.002, 1e-08, 0.9, 0.999), 'tables', ADAM_KEYS),
    ('adam', 'two-equal', 0.0): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.9, 0.999)), ('adam', 0.002, 1e-08, 0.9, 0.999), 'tables', ADAM_KEYS),
    ('adam', 'two-equal', 1e-05): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.9, 0.999)), ('adam', 0.002, 1e-08, 0.9, 0.999), 'tables', ADAM_KEYS),
    ('adam', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('adam', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam', 'table-missing', 0.0): (DENSE, None, ('adam', 0.002, 1e-08, 0.9, 0.999), 'none', ()),
    ('adam', 'table-missing', 1e-05): (DENSE, None, ('adam', 0.002, 1e-08, 0.9, 0.999), 'none', ()),
    ('adam-amsgrad', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-amsgrad', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-amsgrad', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-amsgrad', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-amsgrad', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-amsgrad', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-amsgrad', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-amsgrad', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-wd', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-maximize', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-betas', 'one', 0.0): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.8, 0.99)), ('adam', 0.002, 1e-08, 0.8, 0.99), 'tables', ADAM_KEYS),
    ('adam-betas', 'one', 1e-05): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.8, 0.99)), ('adam', 0.002, 1e-08, 0.8, 0.99), 'tables', ADAM_KEYS),
    ('adam-betas', 'two-equal', 0.0): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.8, 0.99)), ('adam', 0.002, 1e-08, 0.8, 0.99), 'tables', ADAM_KEYS),
    ('adam-betas', 'two-equal', 1e-05): (('lazy', 'adam'), ('adam', (0.002, 1e-08, 0.8, 0.99)), ('adam', 0.002, 1e-08, 0.8, 0.99), 'tables', ADAM_KEYS),
    ('adam-betas', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('adam-betas', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('adam-betas', 'table-missing', 0.0): (DENSE, None, ('adam', 0.002, 1e-08, 0.8, 0.99), 'none', ()),
    ('adam-betas', 'table-missing', 1e-05): (DENSE, None, ('adam', 0.002, 1e-08, 0.8, 0.99), 'none', ()),
    ('rmsprop', 'one', 0.0): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.010000000000000009, 0.99)), None, 'tables', RMS_KEYS),
    ('rmsprop', 'one', 1e-05): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.010000000000000009, 0.99)), None, 'tables', RMS_KEYS),
    ('rmsprop', 'two-equal', 0.0): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.010000000000000009, 0.99)), None, 'tables', RMS_KEYS),
    ('rmsprop', 'two-equal', 1e-05): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.010000000000000009, 0.99)), None, 'tables', RMS_KEYS),
    ('rmsprop', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-momentum', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-centered', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-alpha', 'one', 0.0): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.09999999999999998, 0.9)), None, 'tables', RMS_KEYS),
    ('rmsprop-alpha', 'one', 1e-05): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.09999999999999998, 0.9)), None, 'tables', RMS_KEYS),
    ('rmsprop-alpha', 'two-equal', 0.0): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.09999999999999998, 0.9)), None, 'tables', RMS_KEYS),
    ('rmsprop-alpha', 'two-equal', 1e-05): (('lazy', 'rmsprop'), ('rmsprop', (0.003, 1e-08, 0.09999999999999998, 0.9)), None, 'tables', RMS_KEYS),
    ('rmsprop-alpha', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-alpha', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-alpha', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-alpha', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('rmsprop-wd', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
    ('adamw', 'one', 0.0): (DENSE, None, None, 'none', ()),
    ('adamw', 'one', 1e-05): (DENSE, None, None, 'none', ()),
    ('adamw', 'two-equal', 0.0): (DENSE, None, None, 'none', ()),
    ('adamw', 'two-equal', 1e-05): (DENSE, None, None, 'none', ()),
    ('adamw', 'two-lr', 0.0): (DENSE, None, None, 'none', ()),
    ('adamw', 'two-lr', 1e-05): (DENSE, None, None, 'none', ()),
    ('adamw', 'table-missing', 0.0): (DENSE, None, None, 'none', ()),
    ('adamw', 'table-missing', 1e-05): (DENSE, None, None, 'none', ()),
}


def _optimizer(model, config, layout):
    cls, kw = CONFIGS[config]
    params = list(model.parameters())
    if layout == "one":
        return cls(params, **kw)
    if layout == "table-missing":
        gone = model._plan.table_params[0]
        return cls([p for p in params if p is not gone], **kw)
    # both halves hold tables and dense parameters
    groups = [dict(params=params[0::2]), dict(params=params[1::2])]
    if layout == "two-lr":
        groups[1]["lr"] = kw["lr"] * 0.5
    return cls(groups, **kw)


def observe(config, layout, l2):
    model = build_model(load_golden("deepfm_criteo")["spec"], "cpu", l2=l2)
    plan = model.model_plan()
    opt = _optimizer(model, config, layout)
    model.compile(opt, "binary_crossentropy")
    lazy = (plan.lazy.kind, plan.lazy.hyper) if plan.update[0] == "lazy" else None
    tables = set(id(p) for p in plan.table_params)
    dense = model._dense_update_mode([p for p in model.parameters() if id(p) not in tables])
    names = {id(p): n for n, p in model.named_parameters()}
    held = [p for grp in opt.param_groups for p in grp["params"]]
    with_state = sorted(names[id(p)] for p in held if len(opt.state.get(p, {})) > 0)
    keys = tuple(sorted(set(k for p in held for k in opt.state.get(p, {}))))
    who = {"none": [], "optimizer": sorted(names[id(p)] for p in held),
           "tables": sorted(names[id(p)] for p in plan.table_params)}
    label = [k for k in ("none", "optimizer", "tables") if who[k] == with_state]
    return plan.update, lazy, dense, (label[0] if label else with_state), keys


@pytest.mark.parametrize("l2", L2S)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_update_paths_over_the_optimizer_grid(config, layout, l2):
    assert observe(config, layout, l2) == EXPECTED[config, layout, l2]
