"""What the two native PPO updates share above the C ABI (``ppo.PPOUpdate`` and ``marl_ppo.MarlPPOUpdate`` with
``backend="native"``): the net struct over a model's own storage with its rejection path, and Adam's state, the
scratch and the epoch loop around ``ch_ppo_train`` / ``ch_marl_ppo_train``.  What differs per flavour is a row of
``SB3`` / ``RLLIB``; the losses' hyper-parameters and data stay with the two updates."""
import collections
import ctypes

from . import _lib

# label: the messages' prefix; prefix: the ABI's; Net: the net struct; nets: per MLP, the model's attribute with the
# hidden layers, the one with the head Linear and the stem of the struct's fields (n_<stem>, <stem>, <stem>_weight,
# <stem>_bias); log_std: the model has SB3's free log_std parameter
Flavour = collections.namedtuple("Flavour", "label prefix Net nets log_std")
SB3 = Flavour("native PPO update", "ch_ppo_", _lib.ChPpoNet,
              (("policy_net", "action_net", "pi"), ("value_net_mlp", "value_net", "vf")), True)
RLLIB = Flavour("native MARL PPO update", "ch_marl_ppo_", _lib.ChMarlPpoNet,
                (("actor_encoder", "pi", "actor"), ("critic_encoder", "vf", "critic")), False)


def net_struct(fl, model):
    """The flavour's net struct over ``model``'s own storage, as it is now: it holds raw pointers, so build it again
    after anything that may move a parameter.  Raises ``ValueError`` for an architecture the native update does not
    take (with the library's own reason), and for parameters that are not contiguous float32 on the model's CUDA
    device."""
    import torch
    net = fl.Net()
    net.obs_dim, net.act_dim = model.obs_dim, model.act_dim
    got = [f"obs_dim={model.obs_dim}", f"act_dim={model.act_dim}"]
    for hidden, head, stem in fl.nets:
        layers = [m for m in getattr(model, hidden) if hasattr(m, "weight")]
        if not 1 <= len(layers) <= 2:     # (the struct has room for no more)
            raise ValueError(f"{fl.label}: each MLP must have 1 or 2 hidden layers")
        setattr(net, "n_" + stem, len(layers))
        widths, ws, bs = getattr(net, stem), getattr(net, stem + "_weight"), getattr(net, stem + "_bias")
        for i, m in enumerate(layers + [getattr(model, head)]):
            if i < len(layers):
                widths[i] = m.out_features
            ws[i], bs[i] = m.weight.data_ptr(), m.bias.data_ptr()
        got.append(f"{stem}={list(widths)[:len(layers)]}")
    if fl.log_std:
        net.log_std = model.log_std.data_ptr()
    lib = _lib.lib()
    if getattr(lib, fl.prefix + "param_count")(ctypes.byref(net)) < 0:
        why = (lib.ch_last_error(None) or b"").decode()      # the library's own reason
        raise ValueError(f"{fl.label}: {why} (got {', '.join(got)})")
    for p in model.parameters():
        if not p.is_cuda or p.device != model.device:
            raise ValueError(f"{fl.label}: the model must be on a CUDA device (no CPU path exists)")
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"{fl.label}: parameters must be contiguous float32")
    return net


class NativeState:
    """Adam's state for ``model``'s flat parameters (zero moments, step 0, on the device), the scratch, and the epoch
    loop.  Construction raises as ``net_struct`` does."""

    def __init__(self, fl, model):
        import torch
        net_struct(fl, model)   # raises for an unsupported architecture or a model that is not on the GPU
        n = sum(p.numel() for p in model.parameters())
        self.fl, self.model = fl, model
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=model.device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=model.device)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=model.device)
        self.scratch = None

    def prepare(self, n, batch_size):
        """The net struct over the parameters' storage as it is now (a .to() or .data = ... moves it), with the scratch
        sized for minibatches of ``batch_size`` out of ``n`` rows."""
        import torch
        net = net_struct(self.fl, self.model)
        want = getattr(_lib.lib(), self.fl.prefix + "scratch_size")(ctypes.byref(net), min(batch_size, n))
        if self.scratch is None or self.scratch.numel() < want:
            self.scratch = torch.empty(want, dtype=torch.float32, device=self.model.device)
        return net

    def train(self, hp, data, n_epochs, n, batch_size, draw, stats=None, log=False, opts=None):
        """``n_epochs`` calls of the flavour's ``*_train`` on the current stream of the model's device, each over the
        ``n`` row indices (int64, on the device) that ``draw()`` returns, in minibatches of ``batch_size``.  ``hp`` and
        ``data`` are the flavour's hparams and data structs; ``stats``: None or the per-step statistics' float32
        tensor ``[n_epochs * steps per epoch, k]``.  ``log``: ``*_train_log``, whose ``stats`` are required and
        ``CH_PPO_LOG_STATS`` (SB3 flavour) / ``CH_MARL_PPO_LOG_STATS`` (RLlib flavour) wide.  ``opts`` (SB3 flavour): a
        ``ChPpoOpts`` -- every epoch is a ``ch_ppo_train_opt`` call with it, ``stats`` required and
        ``CH_PPO_OPT_STATS`` wide; the caller has zeroed its stop word.  Returns the number of minibatch steps
        (launched: with ``opts``' KL gate the later ones may not have run)."""
        import torch
        lib, dev = _lib.lib(), self.model.device
        net = self.prepare(n, batch_size)
        # the entry point and what it takes ahead of the row indices
        entry = "train_opt" if opts is not None else "train_log" if log else "train"
        train = getattr(lib, self.fl.prefix + entry)
        lead = [ctypes.byref(x) for x in (net, hp, data) + (() if opts is None else (opts,))]
        nb = (n + batch_size - 1) // batch_size
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for e in range(n_epochs):
                idx = draw()
                _lib.check(train(*lead, idx.data_ptr(), n, batch_size,
                                 self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.step_count.data_ptr(),
                                 None if stats is None else stats[e * nb].data_ptr(), self.scratch.data_ptr(), stream))
                # (idx is freed to torch's caching allocator, which is stream-ordered: the launches read it first)
        return n_epochs * nb
