"""The PPO update of the DTDE driver's shared policy over a device MARL rollout buffer: configs[4]'s training half.

The driver trains RLlib ``PPOConfig()`` with one ``"shared_policy"`` over every agent and RLlib's defaults
(``simulator/DTDECattleHerder.py:62-97``).  ``RLlibActorCritic`` is that module for a flat Box observation under
RLlib's key names: ``encoder.actor_encoder`` (Linear + tanh) -> ``pi`` (2 * act_dim outputs: the DiagGaussian's mean,
then the raw log_std, clamped to +-``log_std_clip`` where it is used) and a separate ``encoder.critic_encoder`` ->
``vf`` (``vf_share_layers=False``).  ``device_nets()`` hands ``DeviceMarlRolloutBuffer.collect`` the same storage, so
the next collection sees every optimiser step.

``MarlPPOUpdate.train`` restates RLlib 2.x's new-API-stack PPO learner with its defaults: the clipped surrogate, the
clipped value loss, the entropy bonus, the KL penalty with its adaptive coefficient, Adam, an optional global-norm
clip; ``num_epochs`` passes over the live rows (``agent_mask == 1``) in minibatches of ``minibatch_size``, advantages
standardised once per call.  RLlib is not installed: parity is unpinned to its source.  One stated divergence: each
epoch's last minibatch is partial, where RLlib's cyclic iterator wraps around to fill it.

``backend="torch"`` (the default, eager autograd) is the reference; ``backend="native"`` (or
``CH_PPO_BACKEND=native``) runs the same minibatch sequence through ``ch_marl_ppo_train`` (csrc/ch_ppo.hip compiled
for this loss and head): three hand-written launches per step on the parameters' own storage.

``log_stats=True`` makes ``train`` also fill ``last_log`` with RLlib's ``learners/shared_policy`` logger keys, from
device-side data read once at the end (native: ``ch_marl_ppo_train_log``); ``train_log.rllib_result`` joins it with a
``MarlEpisodeRing``'s env-runner keys.
"""
import math
import os

from . import _ppo_native
from ._lib import ChMarlPpoData, ChMarlPpoHparams, ChMarlPpoNet, lib as _bind  # noqa: F401  (their old home)

KEYS = ("encoder.actor_encoder.net.mlp", "encoder.critic_encoder.net.mlp", "pi.net.mlp.0", "vf.net.mlp.0")


def _torch():
    import torch
    return torch


class RLlibActorCritic:
    """RLlib's default PPO module for a flat Box observation: two tanh encoders of widths ``hiddens`` (the critic's
    ``vf_hiddens`` if given), ``pi`` Linear(h, 2 * act_dim) and ``vf`` Linear(h, 1); torch's default Linear
    initialisation seeded by ``seed``, with the global CPU and CUDA generators left as they were.  ``device=None`` is
    the current GPU; without one, pass ``device="cpu"`` (the torch backend runs there, the native one does not)."""

    def __init__(self, obs_dim=86, act_dim=4, hiddens=(256, 256), device=None, seed=0, vf_hiddens=None):
        torch = _torch()
        nn = torch.nn
        if device is not None:
            dev = torch.device(device)
        elif torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
        else:
            raise RuntimeError("RLlibActorCritic: no ROCm GPU is visible for the default device; pass device='cpu' "
                               "to build the model on the host (torch backend only)")

        def encoder(widths):
            layers, d = [], obs_dim
            for w in widths:
                layers += [nn.Linear(d, w), nn.Tanh()]
                d = w
            return nn.Sequential(*layers), d

        # nn.Linear's init draws from the default CPU generator: fork it and seed that generator alone
        # (torch.manual_seed would reseed every CUDA generator as well, which the fork does not restore)
        with torch.random.fork_rng(devices=[]):
            torch.default_generator.manual_seed(seed)
            self.actor_encoder, da = encoder(tuple(hiddens))
            self.critic_encoder, dc = encoder(tuple(hiddens if vf_hiddens is None else vf_hiddens))
            self.pi = nn.Linear(da, 2 * act_dim)
            self.vf = nn.Linear(dc, 1)
        self.modules = nn.ModuleList([self.actor_encoder, self.critic_encoder, self.pi, self.vf]).to(dev)
        self.device, self.obs_dim, self.act_dim = dev, int(obs_dim), int(act_dim)

    def parameters(self):
        """Actor encoder (weight, bias per layer), critic encoder, pi, vf: the native update's flat order."""
        return list(self.modules.parameters())

    def state_dict_rllib(self):
        """RLlib's names -> the live tensors (no copies)."""
        sd = {}
        for key, seq in ((KEYS[0], self.actor_encoder), (KEYS[1], self.critic_encoder)):
            for i, m in enumerate(seq):
                if hasattr(m, "weight"):
                    sd[f"{key}.{i}.weight"], sd[f"{key}.{i}.bias"] = m.weight, m.bias
        sd[KEYS[2] + ".weight"], sd[KEYS[2] + ".bias"] = self.pi.weight, self.pi.bias
        sd[KEYS[3] + ".weight"], sd[KEYS[3] + ".bias"] = self.vf.weight, self.vf.bias
        return sd

    def load_weights(self, weights):
        """Copy an ``algo.get_weights()[policy]``-style dict (name -> array, e.g. ``policy_weights.pkl``'s) into the
        parameters, in place.  Every parameter must be present with its shape; other keys
        (``pi.log_std_clip_param_const``) are ignored."""
        torch = _torch()
        with torch.no_grad():
            for k, p in self.state_dict_rllib().items():
                if k not in weights:
                    raise KeyError(f"weights lack {k!r}")
                w = torch.as_tensor(weights[k])
                if tuple(w.shape) != tuple(p.shape):
                    raise ValueError(f"{k}: shape {tuple(w.shape)}, the model's is {tuple(p.shape)}")
                p.copy_(w.to(device=p.device, dtype=p.dtype))
        return self

    def device_nets(self):
        """(policy, value) DevicePolicy over the same storage (``.data``: no autograd):
        ``DevicePolicy.rllib_policy`` / ``rllib_value`` for the two-layer encoders RLlib's keys describe."""
        from .policy import DevicePolicy
        sd = {k: v.data for k, v in self.state_dict_rllib().items()}
        if all(f"{KEYS[i]}.2.weight" in sd for i in (0, 1)):
            return DevicePolicy.rllib_policy(sd, self.device), DevicePolicy.rllib_value(sd, self.device)

        def layers(key, head):
            n = sum(1 for k in sd if k.startswith(key) and k.endswith(".weight"))
            return [(sd[f"{key}.{2 * i}.weight"], sd[f"{key}.{2 * i}.bias"]) for i in range(n)] + \
                [(sd[head + ".weight"], sd[head + ".bias"])]
        return (DevicePolicy(layers(KEYS[0], KEYS[2]), "tanh", None, self.device),
                DevicePolicy(layers(KEYS[1], KEYS[3]), "tanh", None, self.device))

    def dist_inputs(self, obs, log_std_clip=20.0):
        """The DiagGaussian's inputs [rows, 2 * act_dim]: the mean, then log_std = the raw output clamped."""
        torch = _torch()
        z = self.pi(self.actor_encoder(obs))
        A = self.act_dim
        return torch.cat([z[:, :A], torch.clamp(z[:, A:], -log_std_clip, log_std_clip)], dim=1)

    def values(self, obs):
        return self.vf(self.critic_encoder(obs)).flatten()


def marl_ppo_net(model):
    """The ``ch_marl_ppo_net`` over ``model``'s own storage (an ``RLlibActorCritic``), as it is now: it holds raw
    pointers, so build it again after anything that may move a parameter.  Raises ``ValueError`` for an architecture
    the native update does not take, and for parameters that are not contiguous float32 on the model's CUDA device."""
    return _ppo_native.net_struct(_ppo_native.RLLIB, model)


STATS = ("policy_loss", "vf_loss", "entropy", "kl", "grad_norm")
# with log_stats: ch_marl_ppo_train_log's columns
LOG_STATS = STATS + ("vf_loss_unclipped", "total_loss", "vf_explained_var")
# RLlib's learners/shared_policy/* keys that ``last_log`` holds
LOG_KEYS = ("policy_loss", "vf_loss", "vf_loss_unclipped", "vf_explained_var", "entropy", "mean_kl_loss", "total_loss",
            "curr_kl_coeff", "curr_entropy_coeff", "gradients_default_optimizer_global_norm", "num_module_steps_trained")


def explained_variance(y, pred):
    """RLlib's ``explained_variance(y, pred)``: ``max(-1, 1 - var(y - pred) / (var(y) + 1e-6))`` with torch's unbiased
    variances, in the tensors' dtype; NaN for one element (0 / 0), which the max keeps."""
    torch = _torch()

    def var(x):
        d = x - x.mean()
        return (d * d).sum() / (x.numel() - 1)
    return torch.maximum(torch.full_like(y[:1].sum(), -1.0), 1.0 - var(y - pred) / (var(y) + 1e-6))


class MarlPPOUpdate:
    """RLlib's PPO learner update over a ``DeviceMarlRolloutBuffer`` (defaults: RLlib's, which the DTDE driver leaves
    untouched).  ``backend``: ``"torch"`` (eager autograd) or ``"native"`` (``ch_marl_ppo_train``); ``None`` reads
    ``CH_PPO_BACKEND`` (default ``"torch"``).  ``kl_coeff`` is a one-float device tensor, adapted after each
    ``train``; ``stats`` holds the last ``train``'s per-step ``[steps, 5]`` statistics (``STATS``) on the device.
    ``log_stats=True`` (both backends; native: ``ch_marl_ppo_train_log``): ``stats`` is ``[steps, 8]`` (``LOG_STATS``:
    also the unclipped value loss, the total loss and RLlib's ``vf_explained_var`` of each minibatch -- the torch
    backend computes them in the model's dtype, the native one as include/cattleherd.h states), and ``train`` fills
    ``last_log`` with RLlib's ``learners/shared_policy`` keys (``LOG_KEYS``), each the last minibatch's value -- the
    one the KL rule uses -- read with one small copy.  RLlib is not installed: restated from its source, parity
    unpinned."""

    def __init__(self, model, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, clip_param=0.3, vf_clip_param=10.0,
                 vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2, kl_target=0.01, num_epochs=30,
                 minibatch_size=128, grad_clip=None, log_std_clip=20.0, seed=0, backend=None, log_stats=False):
        torch = _torch()
        if backend is None:
            backend = os.environ.get("CH_PPO_BACKEND", "torch")
        if backend not in ("torch", "native"):
            raise ValueError(f"MarlPPOUpdate backend must be 'torch' or 'native', not {backend!r}")
        self.backend, self.model = backend, model
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.clip_param, self.vf_clip_param = float(clip_param), float(vf_clip_param)
        self.vf_loss_coeff, self.entropy_coeff = float(vf_loss_coeff), float(entropy_coeff)
        self.kl_target, self.log_std_clip = float(kl_target), float(log_std_clip)
        self.num_epochs, self.minibatch_size = int(num_epochs), int(minibatch_size)
        self.grad_clip = None if grad_clip is None else float(grad_clip)
        if self.minibatch_size < 1 or self.num_epochs < 1:
            raise ValueError("minibatch_size and num_epochs must be >= 1")
        if backend == "native":
            self._native = _ppo_native.NativeState(_ppo_native.RLLIB, model)   # raises for a model it cannot take
        else:
            self.opt = torch.optim.Adam(model.parameters(), lr=self.lr, betas=self.betas, eps=self.eps)
        self.kl_coeff = torch.full((1,), float(kl_coeff), dtype=torch.float32, device=model.device)
        self.gen = torch.Generator(device=model.device).manual_seed(seed)
        self.stats = None
        self.sgd_steps = 0
        self.log_stats, self.last_log = bool(log_stats), {}

    # ---- the loss (the reference: tests compare the native kernels with this in float64) -------------------------
    def _loss(self, obs, actions, old_log_prob, old_dist, advantages, value_targets):
        """(total loss, [policy loss, value loss, mean entropy, mean KL]) of one minibatch, in the model's dtype; with
        ``log_stats`` the statistics go on with [unclipped value loss, total loss, vf_explained_var]."""
        torch = _torch()
        A = self.model.act_dim
        dist = self.model.dist_inputs(obs, self.log_std_clip)
        mean, log_std = dist[:, :A], dist[:, A:]
        mean_p, log_std_p = old_dist[:, :A], old_dist[:, A:]
        var = torch.exp(2.0 * log_std)
        log_prob = (-((actions - mean) ** 2) / (2.0 * var) - log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        ratio = torch.exp(log_prob - old_log_prob)
        surr = torch.min(advantages * ratio,
                         advantages * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param))
        entropy = (log_std + 0.5 + 0.5 * math.log(2.0 * math.pi)).sum(-1)
        kl = (log_std - log_std_p + (torch.exp(2.0 * log_std_p) + (mean_p - mean) ** 2) / (2.0 * var) - 0.5).sum(-1)
        values = self.model.values(obs)
        vf_unclipped = (values - value_targets) ** 2
        vf = torch.clamp(vf_unclipped, 0.0, self.vf_clip_param)
        total = torch.mean(-surr + self.vf_loss_coeff * vf - self.entropy_coeff * entropy) + \
            self.kl_coeff.to(kl.dtype)[0] * torch.mean(kl)
        stats = [-surr.mean(), vf.mean(), entropy.mean(), kl.mean()]
        if self.log_stats:
            stats += [vf_unclipped.mean(), total, explained_variance(value_targets, values)]
        return total, torch.stack(stats).detach()

    def _sgd(self, data, idx, stats_row):
        """One minibatch step in torch: gather, loss, backward, the optional global-norm clip, Adam."""
        torch = _torch()
        loss, st = self._loss(*(t.index_select(0, idx) for t in data))
        self.opt.zero_grad(set_to_none=False)
        loss.backward()
        params = self.model.parameters()
        if self.grad_clip is not None:
            norm = torch.nn.utils.clip_grad_norm_(params, self.grad_clip)
        else:
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
        self.opt.step()
        stats_row[:4] = st[:4]
        stats_row[4] = norm
        stats_row[5:] = st[4:]

    # ---- one training iteration -----------------------------------------------------------------------------------
    def _prepare(self, rb):
        """The flat buffer, the live rows' indices (one host sync for their count), the sampling policy's dist
        inputs over the buffer and the advantages standardised over the live rows."""
        torch = _torch()
        n_all = rb.T * rb.rows
        obs, act = rb.obs.view(n_all, -1), rb.actions.view(n_all, -1)
        live = torch.nonzero(rb.agent_mask.view(n_all), as_tuple=False).view(-1)
        if live.numel() == 0:
            raise ValueError("MarlPPOUpdate.train: the buffer has no live row (agent_mask is 0 everywhere)")
        A = self.model.act_dim
        if self.backend == "native":
            old = self.model.device_nets()[0].forward(obs)    # ch_mlp_forward with the not-yet-updated weights
            old[:, A:].clamp_(-self.log_std_clip, self.log_std_clip)
        else:
            with torch.no_grad():
                # (dead rows are never gathered: whatever they hold, NaN included, stays in its row)
                old = self.model.dist_inputs(obs, self.log_std_clip)
        adv = rb.advantages.view(n_all)
        a = adv.index_select(0, live)
        adv = (adv - a.mean()) / torch.clamp(a.std(unbiased=False), min=1e-4)
        return (obs, act, rb.log_probs.view(n_all), old, adv, rb.returns.view(n_all)), live

    def _adapt_kl(self, kl):
        """RLlib's rule on the last minibatch's mean KL, as device ops on the coefficient (no host sync)."""
        torch = _torch()
        one = torch.ones_like(self.kl_coeff)
        self.kl_coeff.mul_(torch.where(kl > 2.0 * self.kl_target, 1.5 * one,
                                       torch.where(kl < 0.5 * self.kl_target, 0.5 * one, one)))

    def train(self, rb):
        """``num_epochs`` passes over the buffer's live rows; returns the number of minibatch steps taken."""
        torch = _torch()
        data, live = self._prepare(rb)
        n, bs = live.numel(), self.minibatch_size
        nb = (n + bs - 1) // bs
        steps = self.num_epochs * nb
        self.stats = torch.zeros((steps, len(LOG_STATS if self.log_stats else STATS)), dtype=data[0].dtype,
                                 device=self.model.device)
        if self.backend == "native":
            self._train_native(data, live, n)
        else:
            k = 0
            for _ in range(self.num_epochs):
                perm = live[torch.randperm(n, device=self.model.device, generator=self.gen)]
                for j in range(nb):
                    self._sgd(data, perm[j * bs:min((j + 1) * bs, n)], self.stats[k])
                    k += 1
        self._adapt_kl(self.stats[-1, 3].to(torch.float32))
        self.sgd_steps += steps
        if self.log_stats:
            self._fill_log(n)
        return steps

    def _fill_log(self, n):
        """RLlib's learner record of the call: the last minibatch's statistics and the adapted coefficient, gathered
        on the device and read once.  ``n``: the live rows; every epoch passes over each once (the last minibatch is
        partial), so the module trained on ``n * num_epochs`` rows."""
        torch = _torch()
        host = torch.cat([self.stats[-1].double(), self.kl_coeff.double()]).cpu().numpy()      # the one read
        st = dict(zip(LOG_STATS, host))
        self.last_log = {
            "policy_loss": float(st["policy_loss"]),
            "vf_loss": float(st["vf_loss"]),
            "vf_loss_unclipped": float(st["vf_loss_unclipped"]),
            "vf_explained_var": float(st["vf_explained_var"]),
            "entropy": float(st["entropy"]),
            "mean_kl_loss": float(st["kl"]),
            "total_loss": float(st["total_loss"]),
            "curr_kl_coeff": float(host[-1]),
            "curr_entropy_coeff": self.entropy_coeff,
            "gradients_default_optimizer_global_norm": float(st["grad_norm"]),
            "num_module_steps_trained": int(n) * self.num_epochs,
        }

    def _train_native(self, data, live, n):
        """The same permutations as the torch path, one ch_marl_ppo_train call per epoch on the current stream."""
        torch = _torch()
        dev = self.model.device
        data = tuple(t.contiguous() for t in data)
        for t in data:
            if t.dtype != torch.float32 or t.device != dev:
                raise ValueError("native MARL PPO update: the rollout buffer must be float32 on the model's device")
        hp = ChMarlPpoHparams(self.lr, self.betas[0], self.betas[1], self.eps, self.clip_param, self.vf_clip_param,
                              self.vf_loss_coeff, self.entropy_coeff, self.log_std_clip,
                              self.grad_clip if self.grad_clip is not None else 0.0, self.kl_coeff.data_ptr())
        self._native.train(hp, ChMarlPpoData(*(t.data_ptr() for t in data), data[0].shape[0]), self.num_epochs, n,
                           self.minibatch_size, lambda: live[torch.randperm(n, device=dev, generator=self.gen)],
                           self.stats, log=self.log_stats)

    # Adam's moments over the flat parameters and its step count (native backend)
    exp_avg = property(lambda self: self._native.exp_avg)
    exp_avg_sq = property(lambda self: self._native.exp_avg_sq)
    step_count = property(lambda self: self._native.step_count)
