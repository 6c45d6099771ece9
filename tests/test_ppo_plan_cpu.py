"""The native PPO update's dispatch on the CPU: csrc/ch_ppo.h's step plan (through the host-only ch__ppo_plan) and
csrc/ch_ppo.hip's kernel table (ch__ppo_kernel).  The plan is a pure function of (base flavour, log_stats, KL gate
armed, value clip on) -- and of whether the call is ch_ppo_train_opt at all, whose kernels do not depend on an option
being on -- so which kernels an ABI entry launches, with which update bits and how wide a statistics row, is asserted
here with no device.  tests/test_gpu_ppo_plan.py reads the same rows back after real launches."""
import itertools

import pytest

SB3, RLLIB = 0, 1
# The table restated: (fb, dw, adam, update bits, statistics columns, kernels take the option structs) per ABI entry.
TRAIN = {SB3: ("k_ppo_fb<0>", "k_ppo_dw<0>", "k_ppo_adam<0>", 1, 4, False),
         RLLIB: ("k_ppo_fb<1>", "k_ppo_dw<1>", "k_ppo_adam<1>", 1, 5, False)}
TRAIN_LOG = {SB3: ("k_ppo_fb<2>", "k_ppo_dw<0>", "k_ppo_adam<0>", 3, "CH_PPO_LOG_STATS", False),
             RLLIB: ("k_ppo_fb<3>", "k_ppo_dw<1>", "k_ppo_adam<3>", 3, "CH_MARL_PPO_LOG_STATS", False)}
TRAIN_OPT = {False: ("k_ppo_fb_opt<4>", "k_ppo_dw_opt", "k_ppo_adam_opt", 3, "CH_PPO_OPT_STATS", True),
             True: ("k_ppo_fb_opt<5>", "k_ppo_dw_opt", "k_ppo_adam_opt", 3, "CH_PPO_OPT_STATS", True)}
KERNELS = ("k_ppo_fb<0>", "k_ppo_fb<1>", "k_ppo_fb<2>", "k_ppo_fb<3>", "k_ppo_fb_opt<4>", "k_ppo_fb_opt<5>",
           "k_ppo_dw<0>", "k_ppo_dw<1>", "k_ppo_dw_opt", "k_ppo_sumsq", "k_ppo_adam<0>", "k_ppo_adam<1>", "k_ppo_adam<3>",
           "k_ppo_adam_opt")


def _row(want):
    from cattleherd import _lib
    fb, dw, adam, update, width, opts = want
    return {"fb": fb, "dw": dw, "adam": adam, "update": update, "opts": opts,
            "n_stats": getattr(_lib, width) if isinstance(width, str) else width}


def expected(flavour, log, gate, vclip):
    """The plan of one of the 16 combinations; None: it does not exist."""
    if gate or vclip:
        return None if flavour == RLLIB else _row(TRAIN_OPT[vclip])
    return _row((TRAIN_LOG if log else TRAIN)[flavour])


@pytest.mark.parametrize("flavour,log,gate,vclip", list(itertools.product((SB3, RLLIB), *[(False, True)] * 3)))
def test_plan_is_the_table(flavour, log, gate, vclip):
    from cattleherd import _lib
    want = expected(flavour, log, gate, vclip)
    if want is None:   # options and the gate exist for the SB3 flavour only
        with pytest.raises(_lib.ChError) as e:
            _lib.ppo_plan(flavour, log, gate, vclip)
        assert e.value.code == _lib.CH_ERR_UNSUPPORTED
        return
    p = _lib.ppo_plan(flavour, log, gate, vclip)
    assert p == want
    assert p["update"] == (1 if not log and not p["opts"] else 3)
    assert p["n_stats"] == (_lib.CH_PPO_OPT_STATS if p["opts"] else
                            {SB3: _lib.CH_PPO_LOG_STATS, RLLIB: _lib.CH_MARL_PPO_LOG_STATS}[flavour] if log else
                            {SB3: 4, RLLIB: 5}[flavour])


def test_widths_are_the_headers():
    from cattleherd import _lib
    assert (_lib.CH_PPO_LOG_STATS, _lib.CH_PPO_OPT_STATS, _lib.CH_MARL_PPO_LOG_STATS) == (6, 7, 8)
    assert _lib.ppo_plan(SB3, log=True)["n_stats"] == _lib.CH_PPO_LOG_STATS
    assert _lib.ppo_plan(SB3, gate=True)["n_stats"] == _lib.CH_PPO_OPT_STATS
    assert _lib.ppo_plan(RLLIB, log=True)["n_stats"] == _lib.CH_MARL_PPO_LOG_STATS


@pytest.mark.parametrize("log", [False, True])
def test_train_opt_with_both_options_off_keeps_its_kernels(log):
    """ch_ppo_train_opt with target_kl <= 0 and clip_range_vf <= 0 still runs the option kernels (a NULL stop word)
    and writes rows of CH_PPO_OPT_STATS with the state column."""
    from cattleherd import _lib
    assert _lib.ppo_plan(SB3, log, opts=True) == _row(TRAIN_OPT[False])


@pytest.mark.parametrize("flavour,log,opts,gate,vclip", [(RLLIB, False, True, False, False), (RLLIB, True, True, True, True),
                                                         (SB3, False, False, True, False), (SB3, True, False, False, True),
                                                         (2, False, False, False, False), (-1, True, False, False, False)])
def test_what_does_not_exist_is_rejected(flavour, log, opts, gate, vclip):
    """Options with the RLlib flavour, a gate or a value clip without options, a flavour that is no base."""
    from cattleherd import _lib
    with pytest.raises(_lib.ChError) as e:
        _lib.ppo_plan(flavour, log, gate, vclip, opts=opts)
    assert e.value.code == _lib.CH_ERR_UNSUPPORTED


def test_table_holds_each_kernel_once():
    from cattleherd import _lib
    table = _lib.ppo_kernel_table()
    assert table[0] == "none"
    assert sorted(table[1:]) == sorted(KERNELS) and len(set(table)) == len(KERNELS) + 1
    assert _lib.lib().ch__ppo_kernel(-1) is None and _lib.lib().ch__ppo_kernel(len(table)) is None
    # every row but k_ppo_sumsq (ch_*_adam launches it outside a plan) is reached by some plan
    reached = set()
    for flavour, log, gate, vclip in itertools.product((SB3, RLLIB), *[(False, True)] * 3):
        if expected(flavour, log, gate, vclip) is not None:
            p = _lib.ppo_plan(flavour, log, gate, vclip)
            reached |= {p["fb"], p["dw"], p["adam"]}
    assert reached == set(KERNELS) - {"k_ppo_sumsq"}
