"""The PPO update of the CTDE driver over a device rollout buffer: configs[2]'s training half, for the end-to-end
training rate (collection + update) beside the collection-only rate.

The driver trains ``PPO("MlpPolicy", learning_rate=3e-4, n_steps=2048, batch_size=64, n_epochs=10, gamma=0.99,
gae_lambda=0.95, clip_range=0.1, ent_coef=0.1, vf_coef=0.7, max_grad_norm=0.5, policy_kwargs=dict(log_std_init=-1,
ortho_init=False, net_arch=[dict(pi=[128, 128], vf=[128, 128])]))`` (``simulator/CTDECattleHerder.py:107-127``).
``SB3ActorCritic`` is that ActorCriticPolicy (flatten -> separate tanh MLPs -> ``action_net`` / ``value_net``, a free
``log_std``) with SB3's parameter names; ``device_nets()`` hands the rollout kernels the same storage, so every
optimizer step is seen by the next collection (``DevicePolicy`` re-packs before each forward).  ``PPOUpdate.train``
restates SB3 2.x ``PPO.train``: ``n_epochs`` passes over a fresh permutation of the buffer in minibatches of
``batch_size``, per-minibatch advantage normalisation, the clipped surrogate, MSE value loss, entropy bonus, Adam
(eps 1e-5, SB3's ActorCriticPolicy default), ``clip_grad_norm_``.  SB3 is not installed: parity unpinned to its
source (the permutation comes from torch's generator, not NumPy's).

With ``graph=True`` each run of ``steps_per_graph`` minibatch steps is one captured HIP graph (static index buffer,
capturable Adam): the update of a 64-row minibatch is ~60 small kernels, so launch overhead, not arithmetic, is
what an eager loop would measure.

``backend="native"`` (or ``CH_PPO_BACKEND=native``) runs the same minibatch sequence through ``ch_ppo_train``
(csrc/ch_ppo.hip): forward, loss, backward, ``clip_grad_norm_`` and Adam as three hand-written launches per step, on
the parameters' own storage.  The default stays ``"torch"``.

``log_stats=True`` (native backend) makes ``train`` also fill ``last_log`` with SB3's ``train/`` logger keys, from
device-side data read once at the end: ``ch_ppo_train_log``'s per-minibatch ``approx_kl`` and ``clip_fraction`` beside
the losses, and the buffer's explained variance (``train_log.explained_variance``, float64 where SB3 is float32).

Three more of SB3's ``PPO(...)`` arguments, on both backends: ``target_kl`` (``train`` ends at the first minibatch whose
``approx_kl`` exceeds ``1.5 * target_kl``, before its optimizer step), ``clip_range_vf`` (the value prediction clipped
around the rollout's ``values``) and callable ``learning_rate`` / ``clip_range`` (functions of ``progress_remaining``,
evaluated once per ``train(rb, progress_remaining)``).  The torch backend reads ``approx_kl`` on the host after every
minibatch; the native one runs ``ch_ppo_train_opt``, whose kernels decide on the device -- ``train`` still launches
every step and returns without a synchronisation, and the steps behind the stop return at entry.
"""
import math
import os

from . import _lib, _ppo_native
from ._lib import ChPpoData, ChPpoHparams, ChPpoNet, lib as _bind  # noqa: F401  (the structs' and the binding's old home)


def _torch():
    import torch
    return torch


class SB3ActorCritic:
    """SB3 ``ActorCriticPolicy`` for a flat Box observation: ``mlp_extractor.policy_net`` / ``value_net`` (Linear +
    Tanh, widths ``pi`` / ``vf``), ``action_net``, ``value_net``, ``log_std`` (initialised to ``log_std_init``;
    ``ortho_init=False``: torch's default Linear initialisation)."""

    def __init__(self, obs_dim=1032, act_dim=48, pi=(128, 128), vf=(128, 128), log_std_init=-1.0, device=None,
                 seed=0):
        torch = _torch()
        nn = torch.nn
        g = torch.manual_seed(seed)  # noqa: F841  (default nn.Linear init draws from the global generator)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

        def mlp(widths):
            layers, d = [], obs_dim
            for w in widths:
                layers += [nn.Linear(d, w), nn.Tanh()]
                d = w
            return nn.Sequential(*layers), d

        self.policy_net, dpi = mlp(pi)
        self.value_net_mlp, dvf = mlp(vf)
        self.action_net = nn.Linear(dpi, act_dim)
        self.value_net = nn.Linear(dvf, 1)
        self.log_std = nn.Parameter(torch.ones(act_dim) * log_std_init)
        self.modules = nn.ModuleList([self.policy_net, self.value_net_mlp, self.action_net, self.value_net]).to(dev)
        self.log_std.data = self.log_std.data.to(dev)
        self.device, self.obs_dim, self.act_dim = dev, obs_dim, act_dim

    def parameters(self):
        return list(self.modules.parameters()) + [self.log_std]

    def state_dict_sb3(self):
        """SB3's names -> the live tensors (no copies)."""
        sd = {}
        for i, m in enumerate(self.policy_net):
            if hasattr(m, "weight"):
                sd[f"mlp_extractor.policy_net.{i}.weight"], sd[f"mlp_extractor.policy_net.{i}.bias"] = m.weight, m.bias
        for i, m in enumerate(self.value_net_mlp):
            if hasattr(m, "weight"):
                sd[f"mlp_extractor.value_net.{i}.weight"], sd[f"mlp_extractor.value_net.{i}.bias"] = m.weight, m.bias
        sd["action_net.weight"], sd["action_net.bias"] = self.action_net.weight, self.action_net.bias
        sd["value_net.weight"], sd["value_net.bias"] = self.value_net.weight, self.value_net.bias
        sd["log_std"] = self.log_std
        return sd

    def device_nets(self):
        """(actor mean, critic) DevicePolicy over the same storage (``.data``: no autograd), and the log_std tensor."""
        from .policy import DevicePolicy
        sd = {k: v.data for k, v in self.state_dict_sb3().items()}
        return DevicePolicy.sb3_actor(sd, clip=False), DevicePolicy.sb3_critic(sd), self.log_std.data

    def evaluate_actions(self, obs, actions):
        """SB3 ``evaluate_actions`` with a DiagGaussian: values, summed log-probabilities, summed entropies."""
        torch = _torch()
        mean = self.action_net(self.policy_net(obs))
        values = self.value_net(self.value_net_mlp(obs))
        log_std = self.log_std.expand_as(mean)
        var = torch.exp(2.0 * log_std)
        log_prob = (-((actions - mean) ** 2) / (2.0 * var) - log_std - math.log(math.sqrt(2.0 * math.pi))).sum(-1)
        entropy = (0.5 + 0.5 * math.log(2.0 * math.pi) + log_std).sum(-1)
        return values.flatten(), log_prob, entropy


def ppo_net(model):
    """The ``ch_ppo_net`` over ``model``'s own storage (an ``SB3ActorCritic``), as it is now: it holds raw pointers, so
    build it again after anything that may move a parameter.  Raises ``ValueError`` for an architecture the native
    update does not take, and for parameters that are not contiguous float32 on the model's CUDA device."""
    return _ppo_native.net_struct(_ppo_native.SB3, model)


class PPOUpdate:
    """SB3 ``PPO.train`` over a ``DeviceRolloutBuffer`` (defaults: the CTDE driver's hyper-parameters).
    ``backend``: ``"torch"`` (autograd, optionally graph-captured) or ``"native"`` (``ch_ppo_train``); ``None`` reads
    ``CH_PPO_BACKEND`` (default ``"torch"``).  The native backend ignores ``graph``.  ``log_stats`` (native backend
    only, ``ValueError`` with torch): ``train`` fills ``last_log`` with SB3's ten ``train/`` keys and ``last_stats``
    with the raw per-minibatch statistics ``[steps, 6]`` (ch_ppo_train_log's columns) they were computed from.

    ``target_kl`` / ``clip_range_vf`` (``None``: off, SB3's defaults): see the module text.  With either set the native
    backend runs ``ch_ppo_train_opt`` and ``last_stats`` is its table ``[steps, 7]`` (the seventh column the step's
    state: 1 applied, 0 tripped the gate, -1 not run) after every ``train`` -- read from the device when it is first
    asked for, as ``n_updates`` is (SB3's: the epochs that ran a minibatch) unless ``log_stats`` read it already; the
    torch backend with ``target_kl`` fills the same table on the host (float64, the gradient norm of a tripping row
    NaN: SB3 never forms it).  ``stopped_early`` / ``steps_applied``: whether the last ``train`` tripped the gate, and
    the optimizer steps applied since construction; one synchronisation each on the native backend, on access only.
    ``train``'s return value counts the steps launched there, skipped ones included.  With the torch backend
    ``target_kl`` and callable schedules need ``graph=False`` (``ValueError``): a captured graph can neither stop nor
    change a baked-in scalar.  ``learning_rate`` / ``clip_range`` hold the values of the latest evaluation.  A record
    made through any of these options also carries ``train/learning_rate`` (SB3's ``_update_learning_rate``) and, when
    set, ``train/clip_range_vf``, behind ``LOG_KEYS``."""

    LOG_KEYS = ("train/entropy_loss", "train/policy_gradient_loss", "train/value_loss", "train/approx_kl",
                "train/clip_fraction", "train/loss", "train/explained_variance", "train/std", "train/n_updates",
                "train/clip_range")

    def __init__(self, model, learning_rate=3e-4, n_epochs=10, batch_size=64, clip_range=0.1, ent_coef=0.1,
                 vf_coef=0.7, max_grad_norm=0.5, normalize_advantage=True, graph=True, steps_per_graph=32, seed=0,
                 backend=None, log_stats=False, target_kl=None, clip_range_vf=None):
        torch = _torch()
        if backend is None:
            backend = os.environ.get("CH_PPO_BACKEND", "torch")
        if backend not in ("torch", "native"):
            raise ValueError(f"PPOUpdate backend must be 'torch' or 'native', not {backend!r}")
        self.backend = backend
        self.log_stats = bool(log_stats)
        if self.log_stats and backend != "native":
            raise ValueError("PPOUpdate log_stats=True needs backend='native' (the statistics are ch_ppo_train_log's)")
        self.last_log, self._last_stats, self._n_updates, self._pending, self._epochs_dev = {}, None, 0, None, None
        for name, x in (("target_kl", target_kl), ("clip_range_vf", clip_range_vf)):
            if x is not None and not float(x) > 0.0:
                raise ValueError(f"PPOUpdate {name} must be None or > 0")
        self.target_kl = None if target_kl is None else float(target_kl)
        self.clip_range_vf = None if clip_range_vf is None else float(clip_range_vf)
        # SB3 schedules: functions of progress_remaining, evaluated here at 1.0 and then once per train()
        self._lr_fn = learning_rate if callable(learning_rate) else None
        self._clip_fn = clip_range if callable(clip_range) else None
        learning_rate = float(learning_rate(1.0) if self._lr_fn else learning_rate)
        clip_range = float(clip_range(1.0) if self._clip_fn else clip_range)
        self._opts = self.target_kl is not None or self.clip_range_vf is not None
        self._log_lr = self._opts or self._lr_fn is not None or self._clip_fn is not None
        if backend == "native":
            graph = False
            self._native = _ppo_native.NativeState(_ppo_native.SB3, model)   # raises for a model it cannot take
            self._hp = ChPpoHparams(learning_rate, 0.9, 0.999, 1e-5, clip_range, ent_coef, vf_coef, max_grad_norm,
                                    int(bool(normalize_advantage)), 0)
            self._stop = torch.zeros(1, dtype=torch.int32, device=model.device)   # ch_ppo_train_opt's stop word
        elif graph and self.target_kl is not None:
            raise ValueError("PPOUpdate target_kl with the torch backend needs graph=False (a captured graph cannot stop)")
        elif graph and (self._lr_fn or self._clip_fn):
            raise ValueError("PPOUpdate callable learning_rate / clip_range with the torch backend need graph=False "
                             "(a captured graph holds the values it was captured with)")
        self.model = model
        self.n_epochs, self.batch_size = int(n_epochs), int(batch_size)
        self.learning_rate = learning_rate
        self.clip_range, self.ent_coef, self.vf_coef = clip_range, float(ent_coef), float(vf_coef)
        self.max_grad_norm, self.normalize_advantage = float(max_grad_norm), bool(normalize_advantage)
        self.graph, self.steps_per_graph = bool(graph), int(steps_per_graph)
        if backend == "torch":
            self.opt = torch.optim.Adam(model.parameters(), lr=learning_rate, eps=1e-5, capturable=self.graph)
        self.gen = torch.Generator(device=model.device).manual_seed(seed)
        self._graphs = {}
        self.sgd_steps = 0
        self._stopped, self._applied = False, 0   # (torch backend)

    def _terms(self, obs, actions, old_log_prob, advantages, returns, old_values=None):
        """The loss's three terms (policy loss, value loss, entropy loss) and the log-ratio and ratio they rest on."""
        torch = _torch()
        values, log_prob, entropy = self.model.evaluate_actions(obs, actions)
        if self.normalize_advantage and advantages.shape[0] > 1:
            advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
        log_ratio = log_prob - old_log_prob
        ratio = torch.exp(log_ratio)
        pl = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - self.clip_range, 1 + self.clip_range)).mean()
        if self.clip_range_vf is not None:
            values = old_values + torch.clamp(values - old_values, -self.clip_range_vf, self.clip_range_vf)
        vl = torch.nn.functional.mse_loss(returns, values)
        return pl, vl, -torch.mean(entropy), log_ratio, ratio

    def _loss(self, obs, actions, old_log_prob, advantages, returns, old_values=None):
        pl, vl, el, _, _ = self._terms(obs, actions, old_log_prob, advantages, returns, old_values)
        return pl + self.ent_coef * el + self.vf_coef * vl

    def _sgd(self, data, idx):
        """One minibatch step: gather, loss, backward, clip, Adam (every op on the device, no host sync)."""
        torch = _torch()
        loss = self._loss(*(t.index_select(0, idx) for t in data))
        self.opt.zero_grad(set_to_none=False)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)
        self.opt.step()
        return loss

    def _flat(self, rb):
        T, E = rb.T, rb.obs.shape[1]   # (a population member's buffer has no batch of its own)
        n = T * E
        return (rb.obs.view(n, -1), rb.actions.view(n, -1), rb.log_probs.view(n), rb.advantages.view(n),
                rb.returns.view(n))

    def _graph_for(self, rb, data):
        """A captured run of steps_per_graph minibatch steps over `data`'s storage, reading indices from a static
        [steps_per_graph, batch_size] buffer."""
        torch = _torch()
        key = (id(rb), tuple(t.data_ptr() for t in data))
        g = self._graphs.get(key)
        if g is not None:
            return g
        k, bs = self.steps_per_graph, self.batch_size
        idx = torch.zeros((k, bs), dtype=torch.long, device=self.model.device)
        for p in self.model.parameters():      # gradients exist before capture (zero_grad keeps them)
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        # warm up the captured ops on a side stream (the graph recipe), then undo those steps: the warm-up must not
        # train the model
        saved = [p.detach().clone() for p in self.model.parameters()]
        saved_state = {id(p): {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()}
                       for p, st in self.opt.state.items()}
        s = torch.cuda.Stream(device=self.model.device)
        s.wait_stream(torch.cuda.current_stream(self.model.device))
        with torch.cuda.stream(s):
            for _ in range(2):
                self._sgd(data, idx[0])
        torch.cuda.current_stream(self.model.device).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for j in range(k):
                self._sgd(data, idx[j])
        with torch.no_grad():
            for p, v in zip(self.model.parameters(), saved):
                p.copy_(v)
            for p, st in self.opt.state.items():
                old = saved_state.get(id(p))
                for n, v in st.items():
                    if torch.is_tensor(v):
                        if old is None:
                            v.zero_()            # state the warm-up created: a fresh Adam (step 0, zero moments)
                        else:
                            v.copy_(old[n])
        g = (graph, idx)
        self._graphs[key] = g
        return g

    def _schedules(self, progress_remaining):
        """SB3's ``_update_learning_rate`` and ``clip_range(progress_remaining)``: once per ``train``."""
        if self._lr_fn:
            self.learning_rate = float(self._lr_fn(progress_remaining))
        if self._clip_fn:
            self.clip_range = float(self._clip_fn(progress_remaining))
        if self.backend == "native":
            self._hp.learning_rate, self._hp.clip_range = self.learning_rate, self.clip_range
        elif self._lr_fn:
            for group in self.opt.param_groups:
                group["lr"] = self.learning_rate

    def train(self, rb, progress_remaining=1.0):
        """n_epochs passes over the whole buffer; returns the number of minibatch steps taken (native backend with
        ``target_kl``: launched).  ``progress_remaining``: the schedules' argument (SB3: 1 at the start of learning, 0
        at its end)."""
        torch = _torch()
        self._schedules(progress_remaining)
        data = self._flat(rb)
        n = data[0].shape[0]
        bs = self.batch_size
        nb = (n + bs - 1) // bs
        steps = 0
        if self.backend == "native":
            return self._train_native(data, n, nb, rb)
        if self.clip_range_vf is not None:
            data = data + (rb.values.view(n),)
        if self.target_kl is not None:
            return self._train_gated(data, n, nb)
        for _ in range(self.n_epochs):
            perm = torch.randperm(n, device=self.model.device, generator=self.gen)
            full = n // bs
            j = 0
            if self.graph and full >= self.steps_per_graph:
                graph, idx = self._graph_for(rb, data)
                k = self.steps_per_graph
                while j + k <= full:
                    idx.copy_(perm[j * bs:(j + k) * bs].view(k, bs))
                    graph.replay()
                    j += k
            while j < nb:     # the rest (and a last partial minibatch, as SB3's RolloutBuffer.get yields it)
                self._sgd(data, perm[j * bs:min((j + 1) * bs, n)])
                j += 1
            steps += nb
        self.sgd_steps += steps
        self._applied += steps
        return steps

    def _train_gated(self, data, n, nb):
        """SB3's loop with ``target_kl`` on the torch backend: each minibatch's statistics are read on the host before
        its optimizer step (one synchronisation per step), and the first ``approx_kl > 1.5 * target_kl`` ends the
        call.  Fills ``last_stats`` like ch_ppo_train_opt's table."""
        import numpy as np
        torch = _torch()
        bs, total = self.batch_size, self.n_epochs * nb
        table = np.full((total, _lib.CH_PPO_OPT_STATS), np.nan)
        table[:, 6] = -1.0
        norms, k, self._stopped = [], 0, False
        for e in range(self.n_epochs):
            # (every epoch's permutation is drawn, as the native backend has to: the generator ends where its does)
            perm = torch.randperm(n, device=self.model.device, generator=self.gen)
            if self._stopped:
                continue
            for j in range(nb):
                k = e * nb + j
                pl, vl, el, log_ratio, ratio = self._terms(*(t.index_select(0, perm[j * bs:min((j + 1) * bs, n)]) for t in data))
                loss = pl + self.ent_coef * el + self.vf_coef * vl
                with torch.no_grad():
                    akl = torch.mean((ratio - 1) - log_ratio)
                    cf = torch.mean((torch.abs(ratio - 1) > self.clip_range).to(ratio.dtype))
                    row = torch.stack([pl, vl, -el, akl, cf]).double().cpu().numpy()   # the host read
                table[k, [0, 1, 2, 4, 5]] = row
                if row[3] > 1.5 * self.target_kl:
                    table[k, 6], self._stopped = 0.0, True
                    break
                self.opt.zero_grad(set_to_none=False)
                loss.backward()
                norms.append((k, torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)))
                self.opt.step()
                table[k, 6] = 1.0
            self._n_updates += 1
        if norms:
            table[[i for i, _ in norms], 3] = torch.stack([x for _, x in norms]).double().cpu().numpy()
        self._last_stats = table
        steps = len(norms)
        self.sgd_steps += steps
        self._applied += steps
        return steps

    def _train_native(self, data, n, nb, rb):
        """The same permutations as the torch path, one ch_ppo_train (log_stats: ch_ppo_train_log; with target_kl or
        clip_range_vf: ch_ppo_train_opt) call per epoch on the current stream.  Three parts, of which a population
        (cattleherd/ppo_pop.py) keeps the first and the last: prepare, launch, finish."""
        torch = _torch()
        dev = self.model.device
        stats, opts = self._native_prepare(data, n, nb, rb)
        steps = self._native.train(self._hp, ChPpoData(*(t.data_ptr() for t in data), n), self.n_epochs, n,
                                   self.batch_size, lambda: torch.randperm(n, device=dev, generator=self.gen),
                                   stats=stats, log=self.log_stats, opts=opts)
        return self._native_finish(stats, rb, nb, steps)

    def _native_prepare(self, data, n, nb, rb, pop=False):
        """The rollout's tensors checked, the call's statistics table and its options with the stop word zeroed:
        ``(stats, opts)``, either None when the update has no use for it.  ``pop``: for ch_ppo_train_pop, which goes
        through the option kernels for every member -- always a CH_PPO_OPT_STATS table, always an options struct."""
        torch = _torch()
        dev = self.model.device
        old = rb.values.view(n) if self.clip_range_vf is not None else None
        for t in data + (() if old is None else (old,)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError("native PPO update: the rollout buffer must be contiguous float32 on the model's device")
        stats, opts = None, None
        if self._opts:
            stats = torch.zeros((self.n_epochs * nb, _lib.CH_PPO_OPT_STATS), dtype=torch.float32, device=dev)
            self._stop.zero_()   # (stream-ordered, like the launches behind it)
            opts = _lib.ChPpoOpts(self.target_kl or 0.0, self.clip_range_vf or 0.0, None if old is None else old.data_ptr(),
                                  self._stop.data_ptr() if self.target_kl is not None else None)
        elif pop:
            stats = torch.zeros((self.n_epochs * nb, _lib.CH_PPO_OPT_STATS), dtype=torch.float32, device=dev)
            opts = _lib.ChPpoOpts(0.0, 0.0, None, None)
        elif self.log_stats:
            stats = torch.zeros((self.n_epochs * nb, _lib.CH_PPO_LOG_STATS), dtype=torch.float32, device=dev)
        return stats, opts

    def _native_finish(self, stats, rb, nb, steps, fill_log=True):
        """The bookkeeping behind the launches of ``steps`` minibatch steps: the log, or what ``n_updates`` and
        ``last_stats`` will be read from.  ``fill_log=False``: the caller gathers and records a logging update's
        record itself (a population reads all its members' at once).  Returns ``steps``."""
        self.sgd_steps += steps
        if self.log_stats:
            if fill_log:
                self._fill_log(stats, rb, nb)
        elif self._opts:
            # n_updates and last_stats are read when asked for: the epochs that ran a minibatch are counted on the
            # device (stream-ordered, no synchronisation) and only the latest table is kept
            ran = (stats[:, 6].view(self.n_epochs, nb) >= 0).any(1).sum()
            self._epochs_dev = ran if self._epochs_dev is None else self._epochs_dev + ran
            self._pending = stats
        else:
            self._n_updates += self.n_epochs
        return steps

    def _fill_log(self, stats, rb, nb):
        """SB3 ``PPO.train``'s logger record from the call's statistics, the buffer's explained variance and the
        current ``log_std``: everything is gathered on the device (``_log_gather``) and read once, then recorded
        (``_log_record``)."""
        from .train_log import explained_variance
        ev = explained_variance(rb.values.view(-1), rb.returns.view(-1))
        self._log_record(self._log_gather(stats, ev).cpu().numpy(), stats.shape, nb)      # the one read

    def _log_gather(self, stats, ev):
        """What the record is made of, as one float64 device tensor: the statistics table flattened, ``ev`` (the two
        outputs of the explained variance), the mean standard deviation."""
        torch = _torch()
        std = torch.exp(self.model.log_std.data).mean().double().view(1)
        return torch.cat([stats.double().view(-1), ev.view(-1), std])

    def _log_record(self, host, shape, nb):
        """``last_log``, ``last_stats`` and ``n_updates`` from ``_log_gather``'s tensor on the host (numpy float64; the
        table's ``shape``)."""
        import numpy as np
        from .train_log import sb3_train_record
        size = int(np.prod(shape))
        st = host[:size].reshape(shape)
        self._last_stats = st.astype(np.float32)   # (exact: the values were float32)
        self.last_log, epochs = sb3_train_record(
            st, nb, self.ent_coef, self.vf_coef, self.clip_range, host[size], host[-1], self._n_updates,
            learning_rate=self.learning_rate if self._log_lr else None, clip_range_vf=self.clip_range_vf)
        self._n_updates += epochs

    def _resolve(self):
        """What the ch_ppo_train_opt calls since the last read left on the device (log_stats off): the count of
        epochs that ran a minibatch, and the latest call's table."""
        if self._pending is not None:
            self._last_stats = self._pending.cpu().numpy()
            self._n_updates += int(self._epochs_dev.item())
            self._pending = self._epochs_dev = None

    @property
    def n_updates(self):
        self._resolve()
        return self._n_updates

    @property
    def last_stats(self):
        self._resolve()
        return self._last_stats

    @property
    def stopped_early(self):
        """Whether the last ``train`` ended at the KL gate (native backend: reads the stop word, one synchronisation)."""
        if self.backend != "native":
            return self._stopped
        return self.target_kl is not None and bool(int(self._stop.item()))

    @property
    def steps_applied(self):
        """Optimizer steps applied since construction (native backend: Adam's step count, one synchronisation)."""
        return int(self._native.step_count.item()) if self.backend == "native" else self._applied

    # Adam's moments over the flat parameters and its step count (native backend)
    exp_avg = property(lambda self: self._native.exp_avg)
    exp_avg_sq = property(lambda self: self._native.exp_avg_sq)
    step_count = property(lambda self: self._native.step_count)
