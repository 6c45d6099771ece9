"""The f32 throughput mode (precision="f32", CH_PREC_F32) against the CPU oracle beyond one step of CTDE 4x16 PYB:
under every physics variant, at the shapes and options the f32 path is compared at nowhere else, on the carried
state as well as the outputs, and through in-kernel auto-resets.  tests/test_directed_states_cpu.py holds the census
that keeps these tests from passing vacuously (test_f32_step_census, test_rollout_reference_keeps_its_margins).

A. One f32 step from the directed batch (D.F32_STEP_CASES, 96 envs, the first actions of D.first_actions), per class
   of the batch.  Outputs: the budget of test_f32_throughput_mode_error_budget / test_directed_f32_budget unchanged
   (non-yaw-rate columns 1e-4 / 1e-6, every column within 1e-4 of its scale over the batch, rewards 1e-4 / 1e-6,
   flags exact in every env, roll / pitch rates 1e-4 / 1e-8, yaw rate 3e-4 / 1e-8).  Carried state: integer fields
   exact; every column of every real component within 1e-4 of its scale over the batch, max |device - oracle| /
   max(max |oracle|, floor), the floor that of the observation columns the component feeds (1e-6; 1e-8 for the body
   rates drone_angv and rpy_rates); drone_pos and cow_pos, which an f32 handle carries in f64, by their displacement
   over the step from the injected oracle state, within 1e-4 of the largest oracle displacement of the column.
B. 120 lockstep steps of 16 envs with device Philox actions and auto-reset (D.ROLLOUT_CASES): before every step the
   oracle takes the device state widened exactly.  Actions bit-equal, observations and rewards to the budget of A,
   reset_happened / terminated / truncated equal -- a difference is excused only on an env-step on which a deciding
   quantity of the oracle (D.margins) lies within 1e-4 relative of its threshold, on at most 1 % of the env-steps --
   last_rpm and rpy_rates zero after a reset under a variant, episode and spawn_index exact at the end.
   Neighbour ties (A and B): an observation row lists its drone's two nearest drones in order of distance.  Where
   the oracle's own distances are within 1e-4 relative of each other -- the reset line, whose middle drones have both
   neighbours at exactly 1.75 m, or a regular ring -- the order hangs on a rounding, as a flag on its threshold does:
   such a row is compared with the oracle's row in the tied order nearest to the device's (D.untie_neighbours), to
   the same budget.  The rows so treated are counted, and asserted to be rows of a class that places a regular ring
   (A), or rows of the first ten steps of an episode and at most 1 % of the rows (B).
C. Bit identity where f32 instantiations had none: the v1 kernel against v2 under a physics variant; ch_step_n
   against single steps where f32 has no multi-step kernel.  launch_step_v2_multi<float> (ch_step_multi.hip) exists
   for CTDE 4 x 16 at 16 envs per workgroup only -- tests/test_gpu_directed.py's IDENT holds that one -- so for MARL
   4 x 32 and CTDE 2 x 8 ch_step_n is ch_step n times; the test asserts through ch__multi_steps that it was.

Measured on an MI355X, device against oracle (the figures each test prints):
A, per case, over all classes: the worst observation column against its scale; the worst carried component against
its scale.
  ctde-4x16-L7 physics 1 .. 6   obs 8.0e-7, 9.3e-7, 8.5e-7, 9.3e-7, 1.1e-6, 8.5e-7; state (cow_vel in every case)
                                5.4e-6, 3.6e-6, 4.0e-6, 2.6e-6, 4.0e-6, 3.0e-6
  ctde-6x8-L7 physics 4         obs 5.8e-7; state 2.9e-6
  marl-4x16-L0 physics 5        obs 1.0e-6; state 3.1e-6
  marl-3x8-L0 physics 1         obs 1.6e-6; state 3.1e-6
  ctde-4x32-L7 physics 5 (v1)   obs 1.4e-6; state 4.2e-6
  ctde-8x64-L7 (PW, block 128)  obs 1.6e-6; state 1.1e-5
  ctde-12x16-L7                 obs 1.9e-6; state 3.9e-6
  ctde-3x8-L0 / 4x16-L0 min_drones=2 / 4x16-L4 compat off / 2x8-L7   obs 1.1e-6, 8.0e-7, 6.0e-7, 3.8e-7; state
                                3.3e-6, 2.3e-6, 2.6e-6, 2.5e-6
  Rewards, flags, integer fields and the f64 positions' round trip hold in every case and class, the classes on the
  hold clock included; so do the observation and carried-state bounds, under the downwash variants too (the generator
  staggers the heights there, D._stagger_heights).  One row in the tied neighbour order: the 8-drone `term` ring.
  Misses: 20 body-rate entries (RATE_KNOWN).
B: no flag or reset difference in any case (none excused, none needed); resets 7, 8, 56, 7, 51, 7 (after step ten:
  7, 3, 56, 7, 51, 7); the worst column against its scale 1.3e-5, 1.3e-5, 2.3e-5, 2.0e-5, 1.9e-5, 1.3e-5 (the
  vertical speed, steps 0 and 1); rewards within 1.1e-7 absolute on the last step; rows in the tied order 4, 4, 9, 5,
  0, 4 of 7680 (3840 at 2 x 8), all on the first or second step of an episode; 119 body-rate entries miss their
  elementwise bound, by at most 1.0e-5 rad/s (ROLL_RATE_KNOWN).
"""
import functools

import numpy as np
import pytest

import directed_states as D
from helpers import oracle_view, stack
from test_gpu_directed import (_batch, _device_state, _geometry, _outs, _same_outs, _same_state, _set_kernel, _stagger,
                               _table, _tiled, _worst)

pytestmark = pytest.mark.gpu

CASES = D.F32_STEP_CASES
CLASSES = sorted(set(D.CLASSES))
INT_KEYS = ("step_counter", "step_counter_A", "level", "tally", "has_prev", "spawn_index", "episode")
# real components of the carried state and the floor of the observation columns each feeds
# (test_f32_throughput_mode_error_budget: 1e-6, body rates 1e-8)
DRONE_REAL = {"drone_quat": 1e-6, "drone_vel": 1e-6, "drone_angv": 1e-8, "pid_int_rpy": 1e-6, "pid_int_pos": 1e-6,
              "pid_last_rpy": 1e-6, "drone_qlag": 1e-6}
VARIANT_REAL = {"last_rpm": 1e-6, "rpy_rates": 1e-8}
ENV_REAL = {"cow_vel": 1e-6, "clock": 1e-6, "prev_cent": 1e-6}
BUDGET = 1e-4


@functools.lru_cache(maxsize=None)
def _f32_step(ci):
    """One CH_PREC_F32 step (no auto-reset) from the directed batch and the oracle's step from the same states, with
    the state after it on both sides: computed once per case, shared by the per-class tests, left unchanged."""
    return _f32_step_of(CASES[ci])


def _f32_step_of(case, prepare=None, tobs=False):
    """_f32_step's work for any directed case; ``prepare(batch)`` runs on the new handle before its reset (a geometry
    override, an assertion on its plan).  ``tobs``: the step runs with auto-reset and terminal observations (the only
    way to the kernels that write those); an env that reset is then judged on its terminal observation, reward and
    flags, and its carried state -- the new episode's -- is replaced by the oracle's, i.e. not judged ("reset")."""
    import torch
    mode, n, m, level, kw = case
    E = D.E_DIRECTED
    envs, states = D.directed_states(mode, n, m, level, E, D.case_seed(case), _table(m), **kw)
    bkw = dict(kw)
    if "min_drones" in bkw:
        bkw["max_drones"] = n
    b = _batch(mode, n, m, E, level, precision="f32", **bkw)
    if prepare is not None:
        prepare(b)
    geom = _geometry(b)
    b.reset()
    pre = _device_state(states)
    b.set_state(pre)
    back = b.get_state()
    kept = bool(np.array_equal(back["drone_pos"], pre["drone_pos"][:, :n]) and
                np.array_equal(back["cow_pos"], pre["cow_pos"][:, :m]))
    acts = D.first_actions(states, n, seed=7)
    obs, rew, te, tr = b.step(torch.tensor(acts, device=b.device), autoreset=tobs, terminal_obs=tobs)
    torch.cuda.synchronize()
    reset = b.reset_happened.cpu().numpy().astype(bool) if tobs else np.zeros(E, bool)
    if tobs:
        obs = torch.where(b.reset_happened.bool()[:, None, None], b.terminal_obs, obs)
    out = tuple(x.cpu().numpy() for x in (obs, rew, te, tr))
    g = b.get_state()
    b.close()
    ref = [env.step(acts[e], autoreset=False) for e, env in enumerate(envs)]
    R, K = out[0].shape[1], out[1].shape[1]
    want = (np.stack([r[0] for r in ref]).reshape(E, R, 86), np.stack([r[1] for r in ref]).reshape(E, K),
            np.stack([r[2] for r in ref]).reshape(E, K), np.stack([r[3] for r in ref]).reshape(E, K))
    ws = stack([env.get_state() for env in envs])
    if reset.any():   # (tobs) the new episode's state of an env that reset is not judged: the oracle's in its place
        for k in g:
            if k in ws:
                g[k][reset] = ws[k][reset] if g[k].ndim == 1 else ws[k][reset][:, :g[k].shape[1]]
    ro, ties = D.untie_neighbours(out[0], want[0], ws["n"], lambda e: ws["drone_pos"][e])
    return {"case": case, "reset": reset, "out": out, "want": (ro,) + want[1:], "g": g, "ws": ws, "pre": pre,
            "geom": geom, "kept": kept, "ties": ties,
            "tie_classes": sorted({D.class_of(int(e)) for e, i in np.argwhere((ro != want[0]).any(-1))})}


def _sel(cls):
    return np.array([D.class_of(e) == cls for e in range(D.E_DIRECTED)])


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[D.case_id(c) for c in CASES])
def test_f32_step_route(ci):
    """The kernel ch_create gives the case, and the f64 positions' round trip through set_state / get_state."""
    mode, n, m, level, kw = CASES[ci]
    G, blk, lds, kv = _f32_step(ci)["geom"]
    print(f"ROUTE {D.case_id(CASES[ci])}: G {G} block {blk} lds {lds} kernel v{kv}; observation rows whose two "
          f"nearest drones are tied within 1e-4 and ordered the other way {_f32_step(ci)['ties']} {_f32_step(ci)['tie_classes']}")
    if kw.get("physics", 0) and m > 16:
        assert kv == 1   # a physics variant with more than 16 cows: the v1 kernel
    else:
        assert (G, kv) == (1, 2)
        assert (blk == 128) == (m > 16)   # per-wave tables: the (1, 128) geometry
    assert _f32_step(ci)["kept"]
    # the tied neighbour order only where a class places a regular ring (`ring` when it draws an even one, and the
    # terminating rings of `term` and `levelup`)
    assert set(_f32_step(ci)["tie_classes"]) <= {"ring", "term", "levelup"}, _f32_step(ci)["tie_classes"]


STEP_PARAMS = [(ci, cls) for ci in range(len(CASES)) for cls in CLASSES]
STEP_IDS = [f"{D.case_id(CASES[ci])}-{cls}" for ci, cls in STEP_PARAMS]
STEP = pytest.mark.parametrize("ci,cls", STEP_PARAMS, ids=STEP_IDS)


# Where the budget is missed.  A test below asserts its bound on everything but the entries its table names, so a
# miss anywhere else fails it; the entries themselves are the strict xfail `..._known_misses` test beside it, which
# asserts the same bound on them alone.  Each entry carries the device and the oracle value measured on an MI355X.
#
# Only the elementwise body-rate bounds are missed, as in tests/test_gpu_directed.py's F32_XFAIL.  The f32 step
# leaves an absolute error on a body rate -- the attitude loop's inputs, the PID state and the quaternion, are f32;
# tools/f32_emu.py attributes it, DESIGN.md section 3 -- that these tests measure at up to 1.0e-5 rad/s.  Against the
# columns' scales (rates of up to 6 rad/s) that is within 2.3e-5, which every class and every rollout step asserts;
# elementwise it exceeds 1e-4 (yaw 3e-4) relative on the few entries whose rate is small at that moment: 20 of the
# 5.6e4 rate entries of section A, 119 of the 1.3e5 of section B.  The kernel is left as it is: 1e-4 elementwise needs
# the PID and the quaternion state in f64.  "column 7 / 8 / 9": the roll, pitch and yaw rate; device vs oracle, rad/s.
RATE_KNOWN = {
    "ctde-4x16-L7-physics=4-at1m": {
        "env 81 drone 2 column 7": "7.9411133e-05 vs 7.9528872e-05",
    },
    "ctde-4x16-L7-physics=4-close": {
        "env 20 drone 1 column 8": "-0.0015730102 vs -0.0015732065",
    },
    "ctde-4x16-L7-physics=4-far": {
        "env 69 drone 3 column 9": "8.6241969e-05 vs 8.6186126e-05",
    },
    "ctde-4x16-L7-physics=4-ring": {
        "env 82 drone 2 column 8": "-0.0014502824 vs -0.0014506167",
    },
    "ctde-4x16-L7-physics=5-at1m": {
        "env 81 drone 2 column 7": "-0.00024670945 vs -0.00024686783",
    },
    "ctde-4x16-L7-physics=5-far": {
        "env 53 drone 3 column 8": "-0.00020882017 vs -0.0002087242",
    },
    "ctde-4x16-L7-physics=6-far": {
        "env 21 drone 2 column 8": "-0.00047710538 vs -0.00047687851",
    },
    "marl-4x16-L0-physics=5-oncow": {
        "env 64 drone 3 column 9": "0.00024455987 vs 0.00024465175",
    },
    "marl-3x8-L0-physics=1-oncow": {
        "env 54 drone 0 column 8": "0.00079820305 vs 0.00079830782",
    },
    "ctde-4x32-L7-physics=5-oncow": {
        "env 78 drone 0 column 8": "0.0010540603 vs 0.0010538442",
    },
    "ctde-8x64-L7-far": {
        "env 21 drone 3 column 7": "-0.0035993773 vs -0.003599772",
    },
    "ctde-8x64-L7-levelup": {
        "env 44 drone 1 column 7": "-0.00055911642 vs -0.00055940193",
    },
    "ctde-8x64-L7-oncow": {
        "env 86 drone 5 column 8": "-8.7058637e-05 vs -8.7085333e-05",
    },
    "ctde-12x16-L7-oncow": {
        "env 62 drone 4 column 8": "5.4503535e-06 vs 5.4657799e-06",
        "env 64 drone 3 column 8": "-0.0027656578 vs -0.0027659535",
    },
    "ctde-12x16-L7-ring": {
        "env 2 drone 7 column 9": "-1.5212711e-05 vs -1.527204e-05",
    },
    "ctde-12x16-L7-term": {
        "env 61 drone 9 column 8": "-0.00011750783 vs -0.00011748248",
    },
    "ctde-12x16-L7-trunc_altitude": {
        "env 87 drone 10 column 7": "0.00010270055 vs 0.00010264752",
    },
    "ctde-12x16-L7-trunc_boundary": {
        "env 58 drone 2 column 7": "5.2386578e-05 vs 5.2410789e-05",
        "env 74 drone 8 column 8": "0.00042456944 vs 0.00042471089",
    },
}
ROLL_RATE_KNOWN = {
    "pyb-ctde-4x16": {
        "step 17 env 8 drone 0 column 9": "0.00097274152 vs 0.00097432616",
        "step 24 env 1 drone 1 column 7": "-0.0042519895 vs -0.0042510177",
        "step 30 env 4 drone 0 column 7": "0.0038207138 vs 0.0038255262",
        "step 47 env 8 drone 3 column 8": "0.047995057 vs 0.047988709",
        "step 63 env 11 drone 0 column 8": "0.00016476661 vs 0.00016482543",
        "step 74 env 0 drone 2 column 7": "0.00052137271 vs 0.0005214751",
        "step 81 env 12 drone 2 column 9": "0.0069359932 vs 0.0069414247",
        "step 105 env 1 drone 3 column 9": "-8.9951929e-05 vs -9.2425726e-05",
        "step 105 env 3 drone 0 column 9": "-0.0010846774 vs -0.0010842718",
        "step 114 env 1 drone 1 column 7": "-0.010224787 vs -0.010223571",
        "step 116 env 6 drone 1 column 7": "-0.040041078 vs -0.040045355",
    },
    "pyb-marl-4x16": {
        "step 10 env 8 drone 3 column 9": "-2.4925575e-05 vs -2.5008576e-05",
        "step 14 env 8 drone 0 column 7": "-0.00084915606 vs -0.00084940734",
        "step 24 env 1 drone 1 column 7": "-0.0042519895 vs -0.0042510177",
        "step 45 env 8 drone 2 column 7": "0.0010747525 vs 0.0010745294",
        "step 46 env 6 drone 2 column 7": "-0.0056203888 vs -0.0056209737",
        "step 56 env 0 drone 0 column 9": "-0.019475017 vs -0.019480977",
        "step 78 env 8 drone 1 column 7": "-0.021604106 vs -0.02160628",
        "step 79 env 4 drone 2 column 8": "-0.0027423801 vs -0.00274006",
        "step 83 env 4 drone 2 column 9": "0.00551575 vs 0.0055104266",
        "step 91 env 4 drone 1 column 8": "-0.037993714 vs -0.037988029",
        "step 105 env 1 drone 3 column 9": "-8.9951929e-05 vs -9.2425726e-05",
        "step 105 env 3 drone 0 column 9": "-0.0010846774 vs -0.0010842718",
        "step 111 env 6 drone 0 column 7": "-0.01134121 vs -0.011343173",
        "step 114 env 1 drone 1 column 7": "-0.010224787 vs -0.010223571",
        "step 117 env 8 drone 1 column 7": "0.047918387 vs 0.047928225",
    },
    "dyn-ctde-4x16": {
        "step 0 env 14 drone 0 column 9": "-0.0001271449 vs -0.00012687287",
        "step 1 env 1 drone 1 column 8": "-0.0003975681 vs -0.0003976968",
        "step 1 env 5 drone 1 column 7": "0.0014436216 vs 0.0014437971",
        "step 3 env 6 drone 1 column 8": "0.0038949996 vs 0.0038944012",
        "step 3 env 7 drone 3 column 7": "-0.00030179694 vs -0.00030175355",
        "step 3 env 11 drone 2 column 7": "0.002948422 vs 0.0029488856",
        "step 5 env 4 drone 1 column 8": "0.0025576353 vs 0.0025573394",
        "step 5 env 9 drone 0 column 8": "-0.0024447143 vs -0.0024450168",
        "step 7 env 7 drone 0 column 7": "0.00089467701 vs 0.00089447555",
        "step 13 env 0 drone 3 column 8": "-0.0038203001 vs -0.003820779",
        "step 13 env 1 drone 0 column 9": "-0.00024390221 vs -0.00024401255",
        "step 13 env 7 drone 3 column 9": "0.00014481694 vs 0.00014488724",
        "step 17 env 15 drone 3 column 8": "-0.00030046329 vs -0.00030078579",
        "step 19 env 1 drone 2 column 9": "-0.0001180768 vs -0.0001182116",
        "step 25 env 15 drone 1 column 9": "0.00069701672 vs 0.00069795421",
        "step 31 env 11 drone 0 column 8": "-0.00081056822 vs -0.0008104131",
        "step 32 env 14 drone 3 column 8": "0.0020239151 vs 0.0020236939",
        "step 33 env 2 drone 0 column 9": "-0.00055709865 vs -0.0005573582",
        "step 33 env 7 drone 0 column 7": "0.00022152252 vs 0.00022107147",
        "step 33 env 7 drone 3 column 7": "-0.00086963922 vs -0.00087006",
        "step 33 env 10 drone 1 column 7": "-0.001934588 vs -0.0019351371",
        "step 35 env 4 drone 0 column 7": "-0.00061171968 vs -0.00061188388",
        "step 35 env 4 drone 0 column 8": "0.00024463545 vs 0.00024442951",
        "step 47 env 8 drone 1 column 9": "-0.0014750361 vs -0.0014745281",
        "step 61 env 1 drone 0 column 7": "0.00042759615 vs 0.00042719283",
        "step 64 env 15 drone 0 column 7": "-0.0051517277 vs -0.0051511792",
        "step 65 env 4 drone 2 column 8": "9.0926886e-05 vs 9.1192975e-05",
        "step 65 env 14 drone 3 column 7": "0.0015392415 vs 0.0015388775",
        "step 79 env 15 drone 2 column 8": "0.0018596798 vs 0.0018585479",
        "step 86 env 7 drone 0 column 8": "0.00078066438 vs 0.00078053586",
        "step 91 env 11 drone 3 column 8": "-0.00053713354 vs -0.00053697568",
        "step 92 env 0 drone 3 column 8": "-0.00032931194 vs -0.00032963665",
        "step 98 env 15 drone 2 column 7": "-0.0014066086 vs -0.001406864",
        "step 99 env 1 drone 1 column 8": "0.00054192543 vs 0.00054177345",
        "step 112 env 5 drone 0 column 9": "0.00011898577 vs 0.00011889944",
        "step 119 env 14 drone 3 column 9": "0.00028255256 vs 0.00028270984",
    },
    "pyb_gnd_drag_dw-ctde-4x16": {
        "step 3 env 7 drone 2 column 8": "0.00090243266 vs 0.00090232614",
        "step 5 env 5 drone 0 column 7": "-0.00012163257 vs -0.00012165651",
        "step 5 env 10 drone 0 column 7": "0.0002072499 vs 0.00020745039",
        "step 5 env 14 drone 1 column 7": "0.00063959084 vs 0.00063979853",
        "step 5 env 15 drone 2 column 8": "0.0018068242 vs 0.0018065877",
        "step 9 env 9 drone 2 column 7": "0.00039694487 vs 0.00039679112",
        "step 15 env 13 drone 3 column 8": "-0.0097805019 vs -0.0097823311",
        "step 17 env 8 drone 0 column 9": "0.0001829754 vs 0.00018317997",
        "step 19 env 12 drone 1 column 8": "0.0088792108 vs 0.0088773025",
        "step 19 env 12 drone 2 column 8": "-0.00022341812 vs -0.00022372069",
        "step 22 env 5 drone 1 column 9": "-0.0054319194 vs -0.0054336027",
        "step 37 env 8 drone 1 column 7": "0.00066915655 vs 0.00066924328",
        "step 40 env 12 drone 0 column 8": "-0.00041283129 vs -0.00041299817",
        "step 42 env 15 drone 1 column 9": "0.0017474071 vs 0.0017448132",
        "step 45 env 1 drone 2 column 9": "0.0055118394 vs 0.0055147754",
        "step 47 env 8 drone 3 column 8": "0.0011145321 vs 0.001114102",
        "step 50 env 10 drone 0 column 9": "-0.010450816 vs -0.010442941",
        "step 53 env 12 drone 3 column 9": "-0.00011600975 vs -0.00011585308",
        "step 59 env 10 drone 1 column 8": "-0.00088612671 vs -0.00088594004",
        "step 61 env 9 drone 3 column 8": "0.0016929102 vs 0.0016927195",
        "step 63 env 11 drone 0 column 8": "0.00044293277 vs 0.00044300861",
        "step 67 env 4 drone 1 column 8": "-0.0014854727 vs -0.0014858382",
        "step 69 env 10 drone 2 column 9": "0.0054525412 vs 0.0054471334",
        "step 71 env 3 drone 0 column 8": "-4.9607755e-05 vs -4.964797e-05",
        "step 77 env 5 drone 0 column 8": "-0.025729207 vs -0.025732838",
        "step 77 env 13 drone 2 column 7": "0.0017441494 vs 0.0017443545",
        "step 84 env 10 drone 0 column 7": "-0.083602093 vs -0.08361233",
        "step 86 env 3 drone 2 column 9": "0.018054241 vs 0.018060315",
        "step 94 env 0 drone 3 column 8": "-0.00053053471 vs -0.00053041725",
        "step 95 env 3 drone 2 column 8": "0.050443146 vs 0.050437436",
    },
    "dyn_rk4-ctde-2x8": {
        "step 0 env 14 drone 0 column 9": "-0.00012714493 vs -0.00012687288",
        "step 1 env 5 drone 1 column 7": "0.0013102003 vs 0.0013104245",
        "step 3 env 9 drone 1 column 8": "-5.9045498e-05 vs -5.9209146e-05",
        "step 5 env 8 drone 1 column 7": "-0.0026899055 vs -0.0026895776",
        "step 7 env 7 drone 0 column 8": "0.0022046501 vs 0.0022050282",
        "step 16 env 8 drone 1 column 9": "0.00069341063 vs 0.00069216575",
        "step 17 env 7 drone 1 column 9": "0.00089970231 vs 0.00089916878",
        "step 24 env 1 drone 1 column 8": "-0.0024864078 vs -0.0024868578",
        "step 41 env 1 drone 0 column 8": "-0.00026416779 vs -0.00026404843",
        "step 41 env 9 drone 0 column 7": "0.0010254234 vs 0.0010258098",
        "step 70 env 15 drone 1 column 8": "-0.0018727183 vs -0.0018730308",
        "step 73 env 14 drone 0 column 8": "0.0021747947 vs 0.00217516",
        "step 86 env 7 drone 0 column 8": "0.00098268688 vs 0.00098231714",
        "step 98 env 2 drone 1 column 9": "-0.0012326241 vs -0.0012331881",
        "step 103 env 8 drone 0 column 7": "-0.0054012323 vs -0.0054017962",
        "step 107 env 8 drone 1 column 7": "-0.0010213628 vs -0.0010211678",
    },
    "pyb-ctde-4x32": {
        "step 17 env 8 drone 0 column 9": "0.00097274152 vs 0.00097432616",
        "step 24 env 1 drone 1 column 7": "-0.0042519895 vs -0.0042510177",
        "step 30 env 4 drone 0 column 7": "0.0038207138 vs 0.0038255262",
        "step 47 env 8 drone 3 column 8": "0.047995057 vs 0.047988709",
        "step 63 env 11 drone 0 column 8": "0.00016476661 vs 0.00016482543",
        "step 74 env 0 drone 2 column 7": "0.00052137271 vs 0.0005214751",
        "step 81 env 12 drone 2 column 9": "0.0069359932 vs 0.0069414247",
        "step 105 env 1 drone 3 column 9": "-8.9951929e-05 vs -9.2425726e-05",
        "step 105 env 3 drone 0 column 9": "-0.0010846774 vs -0.0010842718",
        "step 114 env 1 drone 1 column 7": "-0.010224787 vs -0.010223571",
        "step 116 env 6 drone 1 column 7": "-0.040041078 vs -0.040045355",
    },
}


def _new(found, known):
    return {k: v for k, v in found.items() if k not in known}


def _known_params(table):
    return [pytest.param(i, id=i, marks=pytest.mark.xfail(strict=True, reason="; ".join(f"{k}: {v}" for k, v in t.items())))
            for i, t in table.items()]


@STEP
def test_f32_step_flags_and_rewards(ci, cls):
    """Rewards within 1e-4 relative down to 1e-6, terminated and truncated exact, in every env of the class (the
    classes that sit on the hold clock included: D.ON_THRESHOLD)."""
    _check_flags_and_rewards(_f32_step(ci), cls)


def _check_flags_and_rewards(d, cls):
    sel = _sel(cls)
    (_, rew, te, tr), (_, rr, rte, rtr) = [[x[sel] for x in d[k]] for k in ("out", "want")]
    ok_r, w_r = _worst(rew, rr, 1e-4, 1e-6)
    print(f"FLAGS {D.case_id(d['case'])}-{cls}: reward worst (index, device, oracle) {w_r}; flags differ in "
          f"{int((te.astype(bool) != rte.astype(bool)).sum() + (tr.astype(bool) != rtr.astype(bool)).sum())}")
    assert ok_r, ("reward", cls, w_r)
    assert np.array_equal(te.astype(bool), rte.astype(bool)), cls
    assert np.array_equal(tr.astype(bool), rtr.astype(bool)), cls


def _obs_misses(ci, cls):
    return _obs_misses_of(_f32_step(ci), cls)


def _obs_misses_of(d, cls):
    """Observation columns of the class that miss: "col c" elementwise (1e-4 / 1e-6, the yaw rate aside), "scale c"
    against the column's scale over the batch (1e-4) -> worst (device, oracle) or the ratio."""
    sel = _sel(cls)
    o, ro = d["out"][0][sel].astype(np.float64), d["want"][0][sel].astype(np.float64)
    scale = np.maximum(np.abs(d["want"][0]).max(axis=(0, 1)), 1e-6)
    err = (np.abs(o - ro) / scale).max(axis=(0, 1))
    found = {}
    for c in range(86):
        if c != 9:
            ok, w = _worst(o[..., c], ro[..., c], 1e-4, 1e-6)
            if not ok:
                found[f"col {c}"] = f"{w[1]:.8g} vs {w[2]:.8g}"
        if not err[c] <= 1e-4:
            found[f"scale {c}"] = f"{err[c]:.2e} of its scale"
    return found, int(err.argmax()), float(err.max())


@STEP
def test_f32_step_observations(ci, cls):
    """Every observation column but the yaw rate within 1e-4 relative down to 1e-6, and every column within 1e-4
    of its scale over the batch."""
    found, c, worst = _obs_misses(ci, cls)
    i = f"{D.case_id(CASES[ci])}-{cls}"
    print(f"OBS {i}: worst column against its scale {c} at {worst:.2e}; misses {found}")
    assert not found, (cls, found)


def _rate_misses(o, ro, name):
    """Body-rate entries beyond their elementwise bound (roll / pitch 1e-4 / 1e-8, yaw 3e-4 / 1e-8):
    name(index) -> "device vs oracle"."""
    o, ro = np.asarray(o, np.float64), np.asarray(ro, np.float64)
    rtol = np.array([1e-4, 1e-4, 3e-4])
    bad = ~(np.abs(o[..., 7:10] - ro[..., 7:10]) <= 1e-8 + rtol * np.abs(ro[..., 7:10]))
    return {name(ix): f"{o[ix[:-1] + (7 + ix[-1],)]:.8g} vs {ro[ix[:-1] + (7 + ix[-1],)]:.8g}"
            for ix in map(tuple, np.argwhere(bad))}


def _step_rate_misses(ci, cls):
    return _step_rate_misses_of(_f32_step(ci), cls)


def _step_rate_misses_of(d, cls):
    envs = np.flatnonzero(_sel(cls))
    return _rate_misses(d["out"][0][envs], d["want"][0][envs],
                        lambda ix: f"env {int(envs[ix[0]])} drone {ix[1]} column {7 + ix[2]}")


@STEP
def test_f32_step_body_rates(ci, cls):
    """The elementwise body-rate bounds of the budget: roll / pitch rates within 1e-4 relative down to 1e-8, the yaw
    rate within 3e-4 down to 1e-8, on every entry but those RATE_KNOWN names."""
    found = _step_rate_misses(ci, cls)
    i = f"{D.case_id(CASES[ci])}-{cls}"
    print(f"RATE {i}: misses {found}")
    assert not _new(found, RATE_KNOWN.get(i, {})), (cls, _new(found, RATE_KNOWN.get(i, {})))


@pytest.mark.parametrize("i", _known_params(RATE_KNOWN))
def test_f32_step_body_rates_known_misses(i):
    ci, cls = STEP_PARAMS[STEP_IDS.index(i)]
    found = _step_rate_misses(ci, cls)
    assert not set(found) & set(RATE_KNOWN[i]), found


def _scale_rule(dev, ref, mask, sel, floor):
    """Per column (last axis): max over the class's envs of |dev - ref| against max(max over the batch of |ref|,
    floor).  ``mask``: the entries that exist (live drones).  Returns (worst ratio, column, device, oracle)."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    if dev.ndim == 1:
        dev, ref, mask = dev[:, None], ref[:, None], mask[:, None]
    mask = np.broadcast_to(mask if mask.ndim == dev.ndim else mask[..., None], dev.shape)
    lead = tuple(range(dev.ndim - 1))
    scale = np.where(mask, np.abs(ref), 0.0).max(axis=lead)
    diff = np.where(mask, np.abs(dev - ref), 0.0)
    diff = np.where(np.isnan(diff), np.inf, diff)[sel]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0, 0.0, diff / (np.maximum(scale, floor) if floor is not None else scale))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), int(i[-1]), float(dev[sel][i]), float(ref[sel][i])


@STEP
def test_f32_step_integer_state(ci, cls):
    """get_state() after the step: the integer fields and the agents' active bits equal the oracle's."""
    _check_integer_state(_f32_step(ci), cls)


def _check_integer_state(d, cls):
    mode, n, m, level, kw = d["case"]
    g, ws, sel = d["g"], d["ws"], _sel(cls)
    live = np.arange(n)[None, :] < ws["n"][:, None]
    assert np.array_equal(g["n"], ws["n"])
    for k in INT_KEYS:
        assert np.array_equal(g[k][sel], ws[k][sel]), (k, cls, g[k][sel], ws[k][sel])
    assert np.array_equal(g["active"][live & sel[:, None]], ws["active"][:, :n][live & sel[:, None]]), cls


def _state_figures(ci, cls):
    return _state_figures_of(_f32_step(ci), cls)


def _state_figures_of(d, cls):
    """(component, worst ratio against the column's scale, column, device, oracle) of every real component."""
    mode, n, m, level, kw = d["case"]
    g, ws, pre, sel = d["g"], d["ws"], d["pre"], _sel(cls)
    live = np.arange(n)[None, :] < ws["n"][:, None]
    figs = []
    real = dict(DRONE_REAL, **(VARIANT_REAL if kw.get("physics", 0) else {}))
    for k, floor in real.items():
        figs.append((k,) + _scale_rule(g[k], ws[k][:, :n], live, sel, floor))
    ones = np.ones(len(sel), bool)
    figs.append(("cow_vel",) + _scale_rule(g["cow_vel"], ws["cow_vel"][:, :m], ones[:, None], sel, ENV_REAL["cow_vel"]))
    for k in ("clock", "prev_cent"):
        figs.append((k,) + _scale_rule(g[k], ws[k], ones, sel, ENV_REAL[k]))
    # the f64 positions: the displacement over the step from the injected oracle state, against the largest oracle
    # displacement of the column over the batch (no floor: a column in which the oracle does not move at all -- the
    # cattle under DYN -- must not move on the device either)
    p0, c0 = pre["drone_pos"][:, :n], pre["cow_pos"][:, :m]
    figs.append(("d drone_pos",) + _scale_rule(g["drone_pos"] - p0, ws["drone_pos"][:, :n] - p0, live, sel, None))
    figs.append(("d cow_pos",) + _scale_rule(g["cow_pos"] - c0, ws["cow_pos"][:, :m] - c0, ones[:, None], sel, None))
    return figs


@STEP
def test_f32_step_carried_state(ci, cls):
    """get_state() after the step against the oracle's: real components by the column-scale rule, the f64 positions
    by their displacement over the step (module docstring)."""
    figs = _state_figures(ci, cls)
    i = f"{D.case_id(CASES[ci])}-{cls}"
    print(f"STATE {i}: " + "; ".join(f"{k}[{col}] {ratio:.2e} ({dv:.9g} vs {ov:.9g})" for k, ratio, col, dv, ov in figs))
    found = {k: f"column {col} {ratio:.2e} of its scale ({dv:.8g} vs {ov:.8g})" for k, ratio, col, dv, ov in figs
             if not ratio <= BUDGET}
    assert not found, (cls, found)


# ---- B: lockstep rollouts ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rollout(ci):
    """The lockstep rollout of D.ROLLOUT_CASES[ci], run once: what it found, for the tests below to assert."""
    import torch
    import oracle as O
    from cattleherd._lib import PHYSICS
    physics, mode, n, m = D.ROLLOUT_CASES[ci]
    E, T, level, off = D.ROLLOUT_E, D.ROLLOUT_T, D.rollout_level(mode), D.ROLLOUT_OFFSET[D.ROLLOUT_CASES[ci]]
    ph, table = PHYSICS[physics], _table(m)
    mk = lambda e: O.Env(mode, n, m, table, start_level=level, env_id=off + e, physics=ph)   # noqa: E731
    b = _batch(mode, n, m, E, level, precision="f32", physics=physics, env_id_offset=off)
    b.reset()
    envs = [mk(e) for e in range(E)]
    o0 = np.stack([env.reset() for env in envs])
    f = {"reset_obs": _worst(b.obs.cpu().numpy(), o0, 1e-4, 1e-6), "actions": True, "unexcused": [], "excused": [],
         "resets": 0, "later": 0, "obs": (True, None), "scale": (0.0, None), "reward": (True, None), "rates": {},
         "variant_zero": True, "geom": _geometry(b), "ties": 0, "tie_age": [], "rows": 0}
    if mode == 1:
        s = D.rollout_start(b.get_state(), mode, n)
        b.set_state({"drone_pos": s["drone_pos"], "clock": s["clock"]})
    R, K = b.obs_rows, b.reward_cols
    rest = [c for c in range(86) if c not in (7, 8, 9)]   # (the body rates: the stricter floor of their own test)
    dn = np.zeros(E, bool)
    # an env whose flags once differed from the oracle's (excused or not) has left the lockstep -- its episode count,
    # which the reset draws use, may differ from now on -- and is compared no further
    live = np.ones(E, bool)

    def keep(key, res, t):   # the first miss, else the latest worst
        if f[key][0] and res[1] is not None:
            f[key] = (res[0], (t,) + tuple(res[1]))

    for t in range(T):
        g = b.get_state()
        if ph and (dn & live).any():   # the resets of the step before: the carried variant state zeroed
            f["variant_zero"] &= bool(np.all(g["last_rpm"][dn & live] == 0) and np.all(g["rpy_rates"][dn & live] == 0))
        for e, env in enumerate(envs):
            env.set_state(oracle_view(g, e, O.NMAX))
        b.step(random_actions=True, autoreset=True)
        torch.cuda.synchronize()
        acts = b.actions.cpu().numpy()
        ref = []
        for e, env in enumerate(envs):
            a = env.random_actions(t)
            f["actions"] &= bool(np.array_equal(a, acts[e]))
            ref.append(env.step(a, autoreset=True))
        te, tr = b.terminated.cpu().numpy().astype(bool), b.truncated.cpu().numpy().astype(bool)
        got_dn = b.reset_happened.cpu().numpy().astype(bool)
        want_te = np.stack([r[2] for r in ref]).reshape(E, K).astype(bool)
        want_tr = np.stack([r[3] for r in ref]).reshape(E, K).astype(bool)
        dn = np.array([bool(r[4]) for r in ref])
        differ = ((te != want_te).any(1) | (tr != want_tr).any(1) | (got_dn != dn)) & live
        for e in np.flatnonzero(differ):
            # excused only if a deciding quantity of the oracle's own step from this state is within 1e-4 of its threshold
            tmp = mk(e)
            pre = oracle_view(g, e, O.NMAX)
            tmp.set_state(pre)
            tmp.step(acts[e], autoreset=False)
            mg = D.margins(pre, tmp.get_state(), mode, m, level)
            k = min(mg, key=mg.get)
            (f["excused"] if mg[k] < D.MARGIN else f["unexcused"]).append((t, int(e), k, float(mg[k])))
        live &= ~differ
        f["resets"] += int((dn & live).sum())
        f["later"] += int((dn & live).sum()) if t >= 10 else 0
        o_all = b.obs.cpu().numpy()
        before = np.stack([r[0] for r in ref]).reshape(E, R, 86)
        ro, ties = D.untie_neighbours(o_all, before, [env.st.n if live[e] else 0 for e, env in enumerate(envs)],
                                      lambda e: envs[e].get_state()["drone_pos"])
        f["ties"] += ties
        f["rows"] += int(sum(env.st.n for e, env in enumerate(envs) if live[e]))
        # steps since the episode began, of every row taken in the tied order (0: the reset's own observation)
        f["tie_age"] += [int(envs[e].st.step_counter_A) for e, i in np.argwhere((ro != before).any(-1))]
        idx = np.flatnonzero(live)
        o, ro = o_all[idx], ro[idx]
        keep("obs", _worst(o[..., rest], ro[..., rest], 1e-4, 1e-6), t)
        scale = np.maximum(np.abs(ro).max(axis=(0, 1)), 1e-6)
        err = (np.abs(o.astype(np.float64) - ro) / scale).max(axis=(0, 1))
        if err.max() > f["scale"][0]:
            f["scale"] = (float(err.max()), (t, int(err.argmax())))
        keep("reward", _worst(b.reward.cpu().numpy()[idx], np.stack([r[1] for r in ref]).reshape(E, K)[idx], 1e-4, 1e-6), t)
        f["rates"].update(_rate_misses(o, ro, lambda ix: f"step {t} env {int(idx[ix[0]])} drone {ix[1]} column {7 + ix[2]}"))
        if f["unexcused"]:
            break
    st = b.get_state()
    want = stack([env.get_state() for env in envs])
    if ph and (dn & live).any():
        f["variant_zero"] &= bool(np.all(st["last_rpm"][dn & live] == 0) and np.all(st["rpy_rates"][dn & live] == 0))
    f["episode"] = bool(np.array_equal(st["episode"][live], want["episode"][live]))
    f["spawn_index"] = bool(np.array_equal(st["spawn_index"][live], want["spawn_index"][live]))
    f["left"] = int((~live).sum())
    b.close()
    return f


ROLL = range(len(D.ROLLOUT_CASES))
ROLL_IDS = [D.rollout_id(c) for c in D.ROLLOUT_CASES]


@pytest.mark.parametrize("ci", ROLL, ids=ROLL_IDS)
def test_f32_rollout_flags_and_resets(ci):
    """Actions bit-equal; reset_happened, terminated and truncated equal on every env-step on which no deciding
    quantity of the oracle is within 1e-4 of its threshold, the excused ones at most 1 % of the env-steps; resets
    inside the window and after its first ten steps; the variant state zeroed by a reset; episode and spawn_index
    exact at the end."""
    physics, mode, n, m = D.ROLLOUT_CASES[ci]
    f = _rollout(ci)
    print(f"ROLLOUT {ROLL_IDS[ci]}: geometry {f['geom']}; resets {f['resets']} ({f['later']} after step 10); flag "
          f"differences excused {len(f['excused'])} {f['excused']}, not excused {f['unexcused']}")
    if m > 16:
        assert f["geom"][1] == 128 and f["geom"][3] == 2   # per-wave tables
    assert f["actions"]
    assert not f["unexcused"], ("(step, env, nearest quantity, its relative distance)", f["unexcused"])
    assert len(f["excused"]) <= 0.01 * D.ROLLOUT_E * D.ROLLOUT_T and f["left"] == len(f["excused"])
    assert f["resets"] > 0 and f["later"] > 0
    assert f["variant_zero"]
    assert f["episode"] and f["spawn_index"]


@pytest.mark.parametrize("ci", ROLL, ids=ROLL_IDS)
def test_f32_rollout_obs_and_reward(ci):
    """Every step's observations (a resetting env's: the new episode's first, against the oracle's reset) and
    rewards to the budget of section A: every column but the three body rates elementwise, every column against
    its scale; the body rates elementwise in test_f32_rollout_body_rates, to their floor of 1e-8."""
    f = _rollout(ci)
    print(f"ROLLOUT {ROLL_IDS[ci]}: tied neighbour rows ordered the other way {f['ties']} of {f['rows']}, steps into "
          f"their episodes {sorted(f['tie_age'])}; reset obs worst {f['reset_obs'][1]}; obs worst (step, index, device, "
          f"oracle) {f['obs'][1]}; column against its scale {f['scale'][0]:.2e} at (step, column) {f['scale'][1]}; reward "
          f"worst {f['reward'][1]}")
    assert f["reset_obs"][0], f["reset_obs"]
    assert f["obs"][0], f["obs"]
    assert f["scale"][0] <= 1e-4, f["scale"]
    assert f["reward"][0], f["reward"]
    # the tied order only on the reset line, before the first actions have told the two distances apart, and rarely
    assert all(a <= 10 for a in f["tie_age"]) and f["ties"] <= 0.01 * f["rows"], (f["ties"], f["tie_age"])


@pytest.mark.parametrize("ci", ROLL, ids=ROLL_IDS)
def test_f32_rollout_body_rates(ci):
    """The elementwise body-rate bounds over the rollout, roll / pitch 1e-4 / 1e-8 and yaw 3e-4 / 1e-8, on every
    entry of its 120 x 16 env-steps but those ROLL_RATE_KNOWN names."""
    f = _rollout(ci)
    print(f"ROLLRATE {ROLL_IDS[ci]}: {len(f['rates'])} misses {f['rates']}")
    new = _new(f["rates"], ROLL_RATE_KNOWN.get(ROLL_IDS[ci], {}))
    assert not new, new


@pytest.mark.parametrize("i", _known_params(ROLL_RATE_KNOWN))
def test_f32_rollout_body_rates_known_misses(i):
    f = _rollout(ROLL_IDS.index(i))
    assert not set(f["rates"]) & set(ROLL_RATE_KNOWN[i]), f["rates"]



# ---- C: bit identity -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("physics", [5, 1], ids=["pyb_gnd_drag_dw", "dyn"])
def test_f32_variant_v1_v2_bit_identical(physics):
    """40 steps of device Philox actions with auto-reset and terminal observations from the directed batch tiled to
    257 envs, f32 under a physics variant: the v1 kernel against v2, outputs and state bit for bit."""
    import torch
    case = (0, 4, 16, 7, {"physics": physics})
    mode, n, m, level, kw = case
    E, T = 257, 40
    s = _tiled(case, E)
    hs = [_batch(mode, n, m, E, level, precision="f32", physics=physics) for _ in range(2)]
    for h, k in zip(hs, (1, 2)):
        _set_kernel(h, k)
        assert _geometry(h)[3] == k
        h.reset()
        h.set_state(s)
    resets = 0
    for t in range(T):
        outs = []
        for h in hs:
            h.step(random_actions=True, autoreset=True, terminal_obs=True)
            outs.append(_outs(h))
        torch.cuda.synchronize()
        assert _same_outs(*outs), t
        resets += int(outs[0][5].sum())
    assert resets > 0
    _same_state(*hs)
    for h in hs:
        h.close()


@pytest.mark.parametrize("case", [(1, 4, 32, 0, {}), (0, 2, 8, 7, {})], ids=D.case_id)
def test_f32_step_n_equals_single_steps(case):
    """ch_step_n against single steps on an f32 handle at shapes for which launch_step_v2_multi<float> has no kernel
    (MARL 4 x 32 is per-wave tables, CTDE 2 x 8 is not the 4 x 16 geometry: ch_step_multi.hip): ch__multi_steps stays
    where it was, ch_step_n runs ch_step 40 times, and outputs and state agree bit for bit, auto-resets included."""
    import torch
    from cattleherd import _lib
    mode, n, m, level, kw = case
    E, T = 257, 40
    s = _stagger(_tiled(case, E), mode, level)
    hs = [_batch(mode, n, m, E, level, precision="f32") for _ in range(2)]
    for h in hs:
        assert _geometry(h)[3] == 2
        h.reset()
        h.set_state(s)
    m0 = _lib.lib().ch__multi_steps(hs[0].handle)
    hs[0].step_n(T, random_actions=True)
    later = 0
    for t in range(T):
        hs[1].step(random_actions=True, autoreset=True, terminal_obs=False)
        if t >= 2:
            later += int(hs[1].reset_happened.sum())
    torch.cuda.synchronize()
    assert _lib.lib().ch__multi_steps(hs[0].handle) == m0   # no multi-step kernel for this shape in f32
    assert _same_outs(_outs(hs[0]), _outs(hs[1]), skip=(4,))   # (no terminal observations from ch_step_n)
    assert later >= 5
    _same_state(*hs)
    for h in hs:
        h.close()
