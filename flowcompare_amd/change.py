"""Change-map post-processing, the step right after the log-prob path.

Drop-in for `clamp_infs` / `log_prob_to_change` of the reference's test_flow.py:241-275: same names, arguments, in-place
clamping of the inputs and the same AssertionError when the result is not finite.  The arithmetic runs in the HIP library
(`fc_change_map_f32`, csrc/staging.hip); there is no CPU fallback.
"""
import torch

from . import engine


def _as_rows(t):
    if t.dim() == 1:
        return t.unsqueeze(0), True
    if t.dim() != 2:
        raise RuntimeError(f"log-prob tensor must be [N] or [B, N], got {tuple(t.shape)}")
    return t, False


def clamp_infs(tensor):
    """test_flow.py:241-247: every +-inf becomes the smallest non-inf entry of the whole tensor, in place."""
    if tensor.isinf().any():
        work = tensor.contiguous()
        engine.clamp_infs(work)
        if work.data_ptr() != tensor.data_ptr():
            tensor.copy_(work)
        print('Clamping infs!')
    return tensor


def log_prob_to_change(log_prob_1_given_0, log_prob_0_given_0, multiple, hard_cutoff=None):
    """NLL to change scaled from 0 to 1 (test_flow.py:249-275)."""
    l10, squeeze = _as_rows(log_prob_1_given_0)
    l00, _ = _as_rows(log_prob_0_given_0)
    w10, w00 = l10.contiguous(), l00.contiguous()
    had_inf = bool(w10.isinf().any()) or bool(w00.isinf().any())
    out, invalid = engine.change_map(w10, w00, float(multiple), None if hard_cutoff is None else float(hard_cutoff))
    if had_inf:                       # the reference's clamp_infs mutates the caller's tensors
        if w10.data_ptr() != l10.data_ptr():
            l10.copy_(w10)
        if w00.data_ptr() != l00.data_ptr():
            l00.copy_(w00)
        print('Clamping infs!')
    assert not invalid
    return out[0] if squeeze else out


def _counts(name, what, counts, B, device):
    if not (torch.is_tensor(counts) and counts.is_cuda and not counts.is_floating_point() and counts.dtype != torch.bool and tuple(counts.shape) == (B,)):
        raise RuntimeError(f"{name}: {what} must be an integer GPU tensor [B] with B = {B}")
    return counts.to(device=device, dtype=torch.int32).contiguous()


def _real_inf(work, counts):
    """an inf in a real slot of work [B, N] (counts None: every slot)"""
    if counts is None:
        return bool(work.isinf().any())
    real = torch.arange(work.shape[1], device=work.device)[None, :] < counts[:, None]
    return bool((work.isinf() & real).any())


def log_prob_to_change_counts(lp_1_0, counts_1, lp_0_0, counts_0, multiple, hard_cutoff=None):
    """log_prob_to_change for rows of different lengths in a padded layout (`fc_change_map_counts_f32`): scene b owns
    lp_1_0[b, :counts_1[b]] and lp_0_0[b, :counts_0[b]] (integer GPU tensors [B]; counts_0 None = every slot of lp_0_0) and gets, bit for bit,
    log_prob_to_change(lp_1_0[b:b+1, :n1], lp_0_0[b:b+1, :n0]) -- except that clamp_infs takes its minimum over the real slots of the whole
    tensor, as log_prob_to_change takes it over the whole tensor.  Pad slots are neither read nor written, whatever they hold; the returned
    [B, N] is NaN behind every count.  Without hard_cutoff a baseline row needs two values: a shorter one raises, naming the scene."""
    for t in (lp_1_0, lp_0_0):
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2):
            raise RuntimeError("log_prob_to_change_counts: expects [B, N] and [B, N0] log-probs on the GPU (flowcompare_amd has no CPU fallback)")
    B = lp_1_0.shape[0]
    c1 = _counts("log_prob_to_change_counts", "counts_1", counts_1, B, lp_1_0.device)
    c0 = None if counts_0 is None else _counts("log_prob_to_change_counts", "counts_0", counts_0, B, lp_1_0.device)
    w10, w00 = lp_1_0.contiguous(), lp_0_0.contiguous()
    had_inf = _real_inf(w10, c1) or _real_inf(w00, c0)
    out, invalid = engine.change_map_counts(w10, c1, w00, c0, float(multiple), None if hard_cutoff is None else float(hard_cutoff))
    if had_inf:                       # the reference's clamp_infs mutates the caller's tensors
        if w10.data_ptr() != lp_1_0.data_ptr():
            lp_1_0.copy_(w10)
        if w00.data_ptr() != lp_0_0.data_ptr():
            lp_0_0.copy_(w00)
        print('Clamping infs!')
    assert not invalid
    return out


def log_prob_to_change_ragged(log_prob_1_given_0, offsets, log_prob_0_given_0, multiple, hard_cutoff=None, base_counts=None):
    """log_prob_to_change for voxels of different sizes (`fc_change_map_ragged_f32`): log_prob_1_given_0 is flat [offsets[-1]], voxel k owns
    [offsets[k], offsets[k + 1]) (int64 [B + 1], ascending from 0); log_prob_0_given_0 [B, N0] is the sampled self evaluation that sets
    voxel k's threshold.  Per voxel the rules, arithmetic and summation order of log_prob_to_change (with offsets[k] = k * N the same
    bits); clamp_infs acts over each whole tensor, in place.  A voxel without rows contributes nothing.  Returns the flat change.
    base_counts (an integer GPU tensor [B]; `fc_change_map_ragged_counts_f32`): voxel k's baseline is log_prob_0_given_0[k, :base_counts[k]], the
    slots behind it are neither read nor written; without hard_cutoff a baseline needs two values."""
    for t in (log_prob_1_given_0, offsets, log_prob_0_given_0):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("log_prob_to_change_ragged: expects GPU tensors (flowcompare_amd has no CPU fallback)")
    if log_prob_1_given_0.dim() != 1 or log_prob_0_given_0.dim() != 2:
        raise RuntimeError(f"log_prob_to_change_ragged: expects flat [total] and [B, N0] log-probs, got {tuple(log_prob_1_given_0.shape)} and "
                           f"{tuple(log_prob_0_given_0.shape)}")
    w10, w00 = log_prob_1_given_0.contiguous(), log_prob_0_given_0.contiguous()
    c0 = None if base_counts is None else _counts("log_prob_to_change_ragged", "base_counts", base_counts, w00.shape[0], w00.device)
    had_inf = bool(w10.isinf().any()) or _real_inf(w00, c0)
    out, invalid = engine.change_map_ragged(w10, offsets.contiguous(), w00, float(multiple), None if hard_cutoff is None else float(hard_cutoff),
                                            counts_0=c0)
    if had_inf:                       # the reference's clamp_infs mutates the caller's tensors
        if w10.data_ptr() != log_prob_1_given_0.data_ptr():
            log_prob_1_given_0.copy_(w10)
        if w00.data_ptr() != log_prob_0_given_0.data_ptr():
            log_prob_0_given_0.copy_(w00)
        print('Clamping infs!')
    assert not invalid
    return out
