"""Shared pieces of the tests of PPOUpdate's target_kl / clip_range_vf / schedules (test_ppo_opts_cpu.py,
test_gpu_ppo_opts.py): a literal restatement of SB3 2.x PPO.train's gated, value-clipped loop on the project's
evaluate_actions and torch.optim.Adam (any dtype and device; float64 is the reference), a literal restatement of its
logger bookkeeping, and the buffer copy with `values`.  make_model, accept and fake_buffer are ppo_native_ref's."""
import numpy as np
import torch

import ppo_native_ref as R


def fake_buffer(rb, dtype):
    """ppo_native_ref.fake_buffer plus the rollout's value predictions (what clip_range_vf reads)."""
    fb = R.fake_buffer(rb, dtype)
    fb.values = rb.values.detach().clone().to(dtype)
    return fb


def sb3_train(model, data, perms, batch_size, target_kl=None, clip_range_vf=None, learning_rate=3e-4, clip_range=0.1,
              ent_coef=0.1, vf_coef=0.7, max_grad_norm=0.5, opt=None, max_steps=None):
    """SB3's PPO.train, line by line, over `data` = (obs, actions, old_log_prob, advantages, returns, old_values) and
    one permutation per epoch.  Returns the lists SB3's logger averages, per-minibatch extras and the optimizer:
    dict(pg_losses, value_losses, entropy_losses, clip_fractions, approx_kl_divs, loss, n_epochs_counted,
    continue_training, steps_applied, clipped_rows, ratios -- each minibatch's ratios as its step saw them).
    max_steps: stop by hand after that many optimizer steps (the "truncated run" a gated one is compared with)."""
    obs, actions, old_log_prob, advantages, returns, old_values = data
    n = obs.shape[0]
    opt = opt or torch.optim.Adam(model.parameters(), lr=learning_rate, eps=1e-5)
    out = dict(pg_losses=[], value_losses=[], entropy_losses=[], clip_fractions=[], approx_kl_divs=[], loss=None,
               n_updates=0, continue_training=True, steps_applied=0, clipped_rows=[], ratios=[], opt=opt)
    for perm in perms:
        for start in range(0, n, batch_size):
            if max_steps is not None and out["steps_applied"] >= max_steps:
                return out
            idx = perm[start:start + batch_size]
            values, log_prob, entropy = model.evaluate_actions(obs[idx], actions[idx])
            adv = advantages[idx]
            if len(adv) > 1:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            ratio = torch.exp(log_prob - old_log_prob[idx])
            out["ratios"].append(ratio.detach())
            policy_loss_1 = adv * ratio
            policy_loss_2 = adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)
            policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()
            out["pg_losses"].append(policy_loss.item())
            out["clip_fractions"].append(torch.mean((torch.abs(ratio - 1) > clip_range).to(ratio.dtype)).item())
            if clip_range_vf is None:
                values_pred = values
            else:
                values_pred = old_values[idx] + torch.clamp(values - old_values[idx], -clip_range_vf, clip_range_vf)
                out["clipped_rows"].append(((values - old_values[idx]).detach(), idx))
            value_loss = torch.nn.functional.mse_loss(returns[idx], values_pred)
            out["value_losses"].append(value_loss.item())
            entropy_loss = -torch.mean(entropy)
            out["entropy_losses"].append(entropy_loss.item())
            loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
            out["loss"] = loss.item()
            with torch.no_grad():
                log_ratio = log_prob - old_log_prob[idx]
                approx_kl_div = torch.mean((torch.exp(log_ratio) - 1) - log_ratio).cpu().numpy()
                out["approx_kl_divs"].append(float(approx_kl_div))
            if target_kl is not None and approx_kl_div > 1.5 * target_kl:
                out["continue_training"] = False
                break
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
            opt.step()
            out["steps_applied"] += 1
        out["n_updates"] += 1
        if not out["continue_training"]:
            break
    return out


def sb3_logger_record(out, explained_var, std, clip_range, n_updates_before=0, learning_rate=None, clip_range_vf=None):
    """SB3's logger.record calls at the end of PPO.train, from sb3_train's lists."""
    rec = {"train/entropy_loss": float(np.mean(out["entropy_losses"])),
           "train/policy_gradient_loss": float(np.mean(out["pg_losses"])),
           "train/value_loss": float(np.mean(out["value_losses"])),
           "train/approx_kl": float(np.mean(out["approx_kl_divs"])),
           "train/clip_fraction": float(np.mean(out["clip_fractions"])),
           "train/loss": out["loss"],
           "train/explained_variance": float(explained_var),
           "train/std": float(std),
           "train/n_updates": n_updates_before + out["n_updates"],
           "train/clip_range": clip_range}
    if learning_rate is not None:
        rec["train/learning_rate"] = learning_rate
    if clip_range_vf is not None:
        rec["train/clip_range_vf"] = clip_range_vf
    return rec


def table_of(out, steps, ent_coef=0.1, vf_coef=0.7):
    """sb3_train's lists as a ch_ppo_train_opt statistics table [steps, 7] (gradient norm column NaN)."""
    t = np.full((steps, 7), np.nan)
    t[:, 6] = -1.0
    k = len(out["pg_losses"])
    t[:k, 0], t[:k, 1], t[:k, 2] = out["pg_losses"], out["value_losses"], -np.array(out["entropy_losses"])
    t[:k, 4], t[:k, 5] = out["approx_kl_divs"], out["clip_fractions"]
    t[:k, 6] = 1.0
    if not out["continue_training"]:
        t[k - 1, 6] = 0.0
    return t


def perms_of(seed, n, n_epochs, device):
    """The permutations PPOUpdate(seed=seed).train draws on `device`."""
    g = torch.Generator(device=device).manual_seed(seed)
    return [torch.randperm(n, device=device, generator=g) for _ in range(n_epochs)]


def spike_log_probs(log_probs, rows, size=0.6):
    """Synthetic old_log_prob noise: +-size (alternating) added to `rows` of the flat tensor, in place -- the
    minibatch that holds all of them has an approx_kl of ~size^2 / 2, one that holds a few a fraction of that."""
    sign = torch.ones(len(rows), dtype=log_probs.dtype, device=log_probs.device)
    sign[1::2] = -1
    log_probs.view(-1)[rows] += size * sign


def vf_conditions(dv, c):
    """Of a minibatch's `values - old_values` (reference run): the clipped fraction, whether both signs are clipped,
    and the smallest distance of a row from the bound in units of c."""
    return (float((dv.abs() > c).double().mean()), bool((dv > c).any() and (dv < -c).any()),
            float((dv.abs() - c).abs().min() / c))
