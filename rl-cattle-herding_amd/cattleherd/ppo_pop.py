"""A population of native PPO updates advanced together: ``PPOPopulation(updates).train(rbs)`` gives what
``[u.train(rb) for u, rb in zip(updates, rbs)]`` gives, bit for bit, with every epoch's minibatch steps of all members
in one set of launches (``ch_ppo_train_pop``, include/cattleherd.h) instead of one set per member.

The members are ``PPOUpdate(backend="native")`` objects -- seeds, hyper-parameter variants -- and stay usable on their
own.  Each keeps its model, Adam state, generator, schedules, stop word and log; the population owns nothing but the
kernels' argument tables.  Collection is per member (one ``DeviceRolloutBuffer`` each) or ``PopulationRollout``'s.
Members with ``log_stats`` get their records from one ``explained_variance_pop`` call and one host read for the
population.
"""
import ctypes

from . import _lib, _ppo_native
from .ppo import PPOUpdate


class PPOPopulation:
    """``updates``: ``PPOUpdate`` objects with ``backend="native"`` that agree on ``n_epochs``, ``batch_size`` and the
    architecture, all with ``clip_range_vf`` or all without, their models on one device (``ValueError`` otherwise).
    They may differ in everything else: weights, seeds, every hyper-parameter and schedule, ``target_kl``,
    ``log_stats``.  Use it from one stream at a time."""

    def __init__(self, updates):
        updates = list(updates)
        if not updates:
            raise ValueError("PPOPopulation needs at least one update")
        for u in updates:
            if not isinstance(u, PPOUpdate) or u.backend != "native":
                raise ValueError("PPOPopulation members must be PPOUpdate(backend='native') objects")
        first = updates[0]
        arch = self._arch(first)
        for u in updates[1:]:
            if (u.n_epochs, u.batch_size) != (first.n_epochs, first.batch_size):
                raise ValueError("PPOPopulation members must agree on n_epochs and batch_size")
            if self._arch(u) != arch:
                raise ValueError("PPOPopulation members must have the same architecture")
            if (u.clip_range_vf is None) != (first.clip_range_vf is None):
                raise ValueError("PPOPopulation members must all set clip_range_vf or all leave it None")
            if u.model.device != first.model.device:
                raise ValueError("PPOPopulation members' models must be on the same device")
        if len({id(u) for u in updates}) != len(updates) or len({id(u.model) for u in updates}) != len(updates):
            raise ValueError("PPOPopulation members must be distinct updates of distinct models")
        self.updates = updates
        self.device = first.model.device
        self._pop = ctypes.c_void_p()
        _lib.check(_lib.lib().ch_ppo_pop_create(len(updates), self.device.index or 0, ctypes.byref(self._pop)))

    @staticmethod
    def _arch(u):
        net = _ppo_native.net_struct(_ppo_native.SB3, u.model)
        return (net.obs_dim, net.act_dim, tuple(net.pi)[:net.n_pi], tuple(net.vf)[:net.n_vf])

    def train(self, rbs, progress_remaining=1.0):
        """``n_epochs`` passes of every member over its own buffer (``rbs``: one ``DeviceRolloutBuffer`` per member,
        all of one row count), ``n_epochs`` calls of ``ch_ppo_train_pop`` on the current stream.  Returns the list of
        what each member's ``train`` would have returned."""
        import torch
        rbs = list(rbs)
        ups = self.updates
        if len(rbs) != len(ups):
            raise ValueError("PPOPopulation.train takes one rollout buffer per member")
        members = (_lib.ChPpoMember * len(ups))()
        tables, nb, n = [], None, None
        for u, rb, mb in zip(ups, rbs, members):
            u._schedules(progress_remaining)
            data = u._flat(rb)
            if n is not None and data[0].shape[0] != n:
                raise ValueError("PPOPopulation.train: the members' buffers must hold the same number of rows")
            n = data[0].shape[0]
            nb = (n + u.batch_size - 1) // u.batch_size
            stats, opts = u._native_prepare(data, n, nb, rb, pop=True)
            st = u._native
            mb.net, mb.hp, mb.opts = st.prepare(n, u.batch_size), u._hp, opts
            mb.data = _lib.ChPpoData(*(t.data_ptr() for t in data), n)
            mb.m, mb.v, mb.step_dev = st.exp_avg.data_ptr(), st.exp_avg_sq.data_ptr(), st.step_count.data_ptr()
            mb.scratch = st.scratch.data_ptr()
            tables.append(stats)
        first = ups[0]
        perms = []   # every permutation stays alive until the last launch is queued
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for e in range(first.n_epochs):
                for u, mb, stats in zip(ups, members, tables):
                    perms.append(torch.randperm(n, device=self.device, generator=u.gen))
                    mb.idx, mb.stats = perms[-1].data_ptr(), stats[e * nb].data_ptr()
                _lib.check(_lib.lib().ch_ppo_train_pop(self._pop, members, len(ups), n, first.batch_size, stream))
        steps = first.n_epochs * nb
        logging = []   # (update, buffer, table) of the members with log_stats
        for u, rb, stats in zip(ups, rbs, tables):
            # what the member's own entry point would have filled: ch_ppo_train_opt's table for a member with
            # options, ch_ppo_train_log's six columns (the same bits) for one with the log alone, none otherwise
            if not u._opts:
                stats = stats[:, :_lib.CH_PPO_LOG_STATS].contiguous() if u.log_stats else None
            u._native_finish(stats, rb, nb, steps, fill_log=False)
            if u.log_stats:
                logging.append((u, rb, stats))
        if logging:
            # the logging members' records: their explained variances in one set of launches, everything gathered
            # into one device tensor and read once; each member's part is what its own _fill_log reads
            from .train_log import explained_variance_pop
            with torch.cuda.device(self.device):
                evs = explained_variance_pop([rb.values.view(-1) for _, rb, _ in logging],
                                             [rb.returns.view(-1) for _, rb, _ in logging])
                parts = [u._log_gather(stats, evs[k]) for k, (u, _, stats) in enumerate(logging)]
                host = torch.cat(parts).cpu().numpy()      # the one read
            at = 0
            for (u, _, stats), part in zip(logging, parts):
                u._log_record(host[at:at + part.numel()], stats.shape, nb)
                at += part.numel()
        return [steps] * len(ups)

    def close(self):
        """Frees the argument tables (after the stream's work: the launches read them)."""
        if self._pop:
            import torch
            torch.cuda.synchronize(self.device)
            _lib.lib().ch_ppo_pop_destroy(self._pop)
            self._pop = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter shutdown)
            pass
