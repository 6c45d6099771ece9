"""The population update's dispatch on the CPU: csrc/ch_ppo.h's ppo_pop_plan (through the host-only ch__ppo_pop_plan)
and csrc/ch_ppo.hip's kPpoPopTable (ch__ppo_pop_kernel).  The population kernels have a table of their own; the solo
update's 14 rows (tests/test_ppo_plan_cpu.py) know nothing of them."""
import ctypes

import pytest

# The table restated: (fb, dw, adam) by (value clip on).
POP = {False: ("k_ppo_fb_pop<4>", "k_ppo_dw_pop<0>", "k_ppo_adam_pop<0>"),
       True: ("k_ppo_fb_pop<5>", "k_ppo_dw_pop<0>", "k_ppo_adam_pop<0>")}
KERNELS = ("k_ppo_fb_pop<4>", "k_ppo_fb_pop<5>", "k_ppo_dw_pop<0>", "k_ppo_adam_pop<0>")


@pytest.mark.parametrize("vclip", [False, True])
def test_population_plan_is_the_table(vclip):
    from cattleherd import _lib
    assert _lib.ppo_pop_plan(vclip) == dict(zip(("fb", "dw", "adam"), POP[vclip]))
    # the flavours are those of the solo plan for the same call
    assert _lib.ppo_pop_plan(vclip)["fb"][-3:] == _lib.ppo_plan(0, vclip=vclip, opts=True)["fb"][-3:]


def test_population_table_holds_each_kernel_once():
    from cattleherd import _lib
    table = _lib.ppo_pop_kernel_table()
    assert sorted(table) == sorted(KERNELS) and len(set(table)) == len(KERNELS)
    L = _lib.lib()
    assert L.ch__ppo_pop_kernel(-1) is None and L.ch__ppo_pop_kernel(len(table)) is None
    reached = set()
    for vclip in (False, True):
        reached |= set(_lib.ppo_pop_plan(vclip).values())
    assert reached == set(KERNELS)
    assert L.ch__ppo_pop_plan(0, None) == _lib.CH_ERR_INVALID


def test_solo_table_is_still_the_14_rows():
    from cattleherd import _lib
    table = _lib.ppo_kernel_table()
    assert len(table) == 15 and table[0] == "none" and not any("pop" in k for k in table)
    assert not set(table) & set(_lib.ppo_pop_kernel_table())


def test_member_struct_layout_is_the_header():
    """ch_ppo_member: the four structs by value, then six pointers."""
    from cattleherd import _lib
    M = _lib.ChPpoMember
    assert M.net.offset == 0 and M.hp.offset == ctypes.sizeof(_lib.ChPpoNet)
    assert M.data.offset == M.hp.offset + ctypes.sizeof(_lib.ChPpoHparams)
    assert M.opts.offset == M.data.offset + ctypes.sizeof(_lib.ChPpoData)
    assert M.idx.offset == M.opts.offset + ctypes.sizeof(_lib.ChPpoOpts)
    assert ctypes.sizeof(M) == M.idx.offset + 6 * 8


def test_population_host_checks_need_no_device():
    """The object-free rejections come before any device call."""
    from cattleherd import _lib
    L = _lib.lib()
    assert L.ch_ppo_pop_create(0, 0, ctypes.byref(ctypes.c_void_p())) == _lib.CH_ERR_INVALID
    assert L.ch_last_error(None).startswith(b"ch_ppo_pop_create: ")
    assert L.ch_ppo_pop_create(2, 0, None) == _lib.CH_ERR_INVALID
    assert L.ch_ppo_train_pop(None, None, 1, 64, 64, None) == _lib.CH_ERR_INVALID
    assert L.ch_last_error(None).startswith(b"ch_ppo_train_pop: ")
    assert L.ch_ppo_pop_destroy(None) == _lib.CH_ERR_INVALID
