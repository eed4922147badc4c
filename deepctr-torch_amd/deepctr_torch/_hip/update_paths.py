"""Which compiled optimizers the O(batch) / fused update paths reproduce EXACTLY, and the walk over a model's
regularisers -- the two questions every path selector of ``BaseModel`` and of the multi-GPU trainers asks.  Host-side and
pure: torch only, no library load, no optimizer state created."""
import torch

_PLAIN = {  # per optimizer class: (kind, hyper-parameters that must agree across groups, switches that must be off)
    torch.optim.SGD: ("sgd", (), ("momentum", "nesterov")),
    torch.optim.Adagrad: ("adagrad", ("eps",), ("lr_decay",)),
    torch.optim.RMSprop: ("rmsprop", ("eps", "alpha"), ("momentum", "centered", "capturable")),
    torch.optim.Adam: ("adam", ("eps", "betas"), ("amsgrad", "capturable", "fused")),
}


def match_optimizer(opt, params):
    """``("sgd", lr)`` / ``("adagrad", lr, eps)`` / ``("rmsprop", lr, eps, alpha)`` / ``("adam", lr, eps, beta1, beta2)``
    (floats) when ``opt`` is a plain SGD / Adagrad / RMSprop / Adam over every one of ``params`` with ONE set of
    hyper-parameters across their groups -- rows with zero gradient then move (or stay) by a closed form the kernels
    replay -- else ``None``.  Plain: exactly the class (AdamW is not Adam), no weight_decay, no maximize, and per class
    the switches of ``_PLAIN``; Adagrad's ``sum`` must already exist (torch creates it at construction)."""
    if opt is None or not params or type(opt) not in _PLAIN:
        return None
    kind, equal, off = _PLAIN[type(opt)]
    group_of = {}
    for grp in opt.param_groups:
        for p in grp["params"]:
            group_of[id(p)] = grp
    groups = {}
    for p in params:
        g = group_of.get(id(p))
        if g is None:
            return None
        groups[id(g)] = g
    g0 = group_of[id(params[0])]
    for g in groups.values():
        if any(g.get(k) != g0.get(k) for k in ("lr",) + equal) or \
                any(g.get(k, 0) for k in ("weight_decay", "maximize") + off):
            return None
    if kind == "adagrad" and not all("sum" in opt.state.get(p, {}) for p in params):
        return None
    hyper = [g0["lr"]]
    for k in equal:
        hyper.extend(g0[k] if k == "betas" else (g0[k],))
    return (kind,) + tuple(float(x) for x in hyper)


def regularizers(model):
    """``(param, l1, l2)`` for every entry of ``model.regularization_weight``, in registration order (entries may be
    ``named_parameters()``' ``(name, tensor)`` tuples; a parameter registered twice is yielded twice)."""
    for weight_list, l1, l2 in model.regularization_weight:
        for w in weight_list:
            yield (w[1] if isinstance(w, tuple) else w), l1, l2
