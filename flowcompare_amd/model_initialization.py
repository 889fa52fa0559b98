"""Drop-in counterpart of the reference's model_initialization.py for the forward log-prob path.

Same public functions, arguments, return values, derived-config side effects and
exceptions as the reference (model_initialization.py:18-245):

    initialize_flow(config, device='cuda', mode='train') -> {'parameters','flow','input_embedder'}
    inner_loop(batch, models_dict, config)               -> (loss, log_prob[B,N], bpd)
    make_sample(n_points, extract_0, models_dict, config, sample_distrib=None, extra_context=None)
    save_flow(model_dict, config, optimizer, scheduler, save_path) / load_flow(load_dict, models_dict)

The modules are parameter containers with the reference's checkpoint names
(flowcompare_amd/modules.py); all arithmetic happens in the HIP engine.
"""
import math

import torch
from torch import nn

from . import modules as M


def load_flow(load_dict, models_dict):
    """model_initialization.py:18-23."""
    models_dict["input_embedder"].load_state_dict(load_dict["input_embedder"])
    models_dict["flow"].load_state_dict(load_dict["flow"])
    return models_dict


def save_flow(model_dict, config, optimizer, scheduler, save_path):
    """model_initialization.py:25-28 (config may be a wandb Config with ._items or a plain dict)."""
    save_dict = {"config": getattr(config, "_items", config),
                 "optimizer": optimizer.state_dict() if optimizer is not None else None,
                 "flow": model_dict["flow"].state_dict(),
                 "input_embedder": model_dict["input_embedder"].state_dict(),
                 "scheduler": scheduler.state_dict() if scheduler is not None else None}
    torch.save(save_dict, save_path)


def initialize_flow(config, device="cuda", mode="train"):
    """model_initialization.py:30-202."""
    X = 1 if config["extra_z_value_context"] else 0
    config["extra_context_dim"] = X
    config["using_extra_context"] = X > 0
    config["global"] = config["input_embedder"] in ["DGCNNembedderGlobal"]

    if config["coupling_block_nonlinearity"] not in ("ELU", "RELU", "GELU"):
        raise Exception("Invalid coupling_block_nonlinearity")
    act = config["coupling_block_nonlinearity"]

    def attn():
        return M.get_cross_attn(config["attn_dim"], config["attn_input_dim"], config["input_embedding_dim"],
                                config["cross_heads"], config["cross_dim_head"], config["attn_dropout"])

    D, Din = config["latent_dim"], config["input_dim"]
    if D > Din:
        if config["augmenter_dist"] == "ConditionalNormal" and config["use_attn_augment"]:
            net = M.MLP(config["attn_dim"] + Din + X, config["net_augmenter_dist_hidden_dims"], (D - Din) * 2, act)
            aug = M.Augment(M.ConditionalNormal(net), x_size=Din, use_context=True)
            augmenter = M.AugmentAttentionPreconditioner(aug, attn, M.MLP(Din, config["hidden_dims"], config["attn_input_dim"], act))
        elif config["augmenter_dist"] in ("ConditionalNormal", "StandardNormal"):
            # The reference builds a bare Augment here whose forward() cannot take the extra_context
            # keyword Flow.log_prob passes: it is not a working configuration there either.
            raise Exception("augmenter without use_attn_augment is not a working reference configuration (Augment.forward "
                            "rejects extra_context); use use_attn_augment: true or latent_dim == input_dim")
        else:
            raise Exception("Invalid augmenter_dist")
    elif D == Din:
        augmenter = M.IdentityTransform()
    else:
        raise Exception("Latent dim < Input dim")

    if config["flow_type"] == "AffineCoupling":
        def flow_for_cif(input_dim, context_dim):
            return M.AffineCoupling(input_dim, config["hidden_dims"], act, context_dim=context_dim,
                                    scale_fn_type=config["affine_scale_fn"])
    elif config["flow_type"] == "ExponentialCoupling":
        def flow_for_cif(input_dim, context_dim):
            return M.ExponentialCoupling(input_dim, config["hidden_dims"], act, context_dim=context_dim,
                                         eps_expm=config["eps_expm"], algo=config["coupling_expm_algo"])
    elif config["flow_type"] == "RationalQuadraticSplineCoupling":
        def flow_for_cif(input_dim, context_dim):
            return M.RationalQuadraticSplineCoupling(input_dim, config["hidden_dims"], act, config["num_bins_spline"],
                                                     context_dim=context_dim)
    else:
        raise Exception("Invalid flow type")

    def pre_attention_mlp(in_dim):
        return M.MLP(in_dim, config["pre_attention_mlp_hidden_dims"], config["attn_input_dim"], act, residual=True)

    ptype = config["permuter_type"]
    if ptype == "ExponentialCombiner":
        permuter = lambda dim: M.ExponentialCombiner(dim, eps_expm=config["eps_expm"])
    elif ptype == "random_permute":
        permuter = lambda dim: M.Permuter(torch.randperm(dim, dtype=torch.long))
    elif ptype == "LinearLU":
        permuter = lambda dim: M.LinearLU(dim, eps=config["linear_lu_eps"])
    elif ptype == "FullCombiner":
        permuter = lambda dim: M.FullCombiner(dim)
    else:
        raise Exception(f"Invalid permuter type: {ptype}")

    transforms = [augmenter]
    L = config["n_flow_layers"]
    for index in range(L):
        transforms.append(M.cif_helper(config, flow_for_cif, attn, pre_attention_mlp))
        if index != L - 1:                      # no ActNorm / permuter after the last coupling
            if config["act_norm"]:
                transforms.append(M.ActNormBijectionCloud(D, data_dep_init=True))
            transforms.append(permuter(D))

    base_dist = M.StandardNormal(shape=(config["sample_size"], D))
    sample_dist = M.Normal(torch.zeros(1), torch.ones(1) * 0.6, shape=(config["sample_size"], D))
    flow = M.Flow(transforms, base_dist, sample_dist, config=config)

    emb = config["input_embedder"]
    if emb == "DGCNNembedder":
        input_embedder = M.DGCNNembedder(emb_dim=config["input_embedding_dim"], n_neighbors=config["n_neighbors"],
                                         out_mlp_dims=config["hidden_dims_embedder_out"])
    elif emb == "DGCNNembedderGlobal":
        input_embedder = M.DGCNNembedderGlobal(input_dim=Din, out_mlp_dims=config["hidden_dims_embedder_out"],
                                               n_neighbors=config["n_neighbors"], emb_dim=config["input_embedding_dim"])
    elif emb == "PAConv":
        input_embedder = M.PointNet2SSGSeg(c=Din - 3, k=config["input_embedding_dim"], out_mlp_dims=config["hidden_dims_embedder_out"])
    elif emb == "idenity":                      # sic, model_initialization.py:173
        input_embedder = nn.Identity()
    else:
        raise Exception("Invalid input embeder!")

    if mode == "train":
        input_embedder.train()
        flow.train()
        if isinstance(input_embedder, M.PointNet2SSGSeg) and not M.PointNet2SSGSeg.TRAINABLE:
            # the PAConv embedder has inference kernels only: it stays frozen in eval() mode (running-statistics BatchNorm) and
            # receives no gradient; the flow on top of it trains
            input_embedder.eval()
            input_embedder.requires_grad_(False)
    else:
        input_embedder.eval()
        flow.eval()
    sharded = False
    if config["data_parallel"]:
        # model_initialization.py:186-188 wraps both modules in nn.DataParallel (one process, one thread per GPU).  Here the same request means
        # scene sharding with ONE PROCESS PER GPU (flowcompare_amd/shard.py: this rank's scenes on its own device, no data-path collective, RCCL
        # only for the loss scalar and the gradient all-reduce): under `python -m torch.distributed.run --nproc-per-node N` every rank builds the
        # same replica on its LOCAL_RANK's device and inner_loop shards the global batch; outside a process group there is nothing to shard over.
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("config['data_parallel'] is true but no torch.distributed process group is initialised: flowcompare_amd shards scenes with one "
                               "process per GPU -- launch with `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` and "
                               "call torch.distributed.init_process_group('nccl') before initialize_flow (nn.DataParallel's one-process threading, "
                               "model_initialization.py:186-188, has no counterpart here)")
        sharded = True
    input_embedder = input_embedder.to(device)
    flow = flow.to(device)

    parameters = list(input_embedder.parameters()) + list(flow.parameters())
    print(f"Number of trainable parameters: {sum(p.numel() for p in parameters)}")
    md = {"parameters": parameters, "flow": flow, "input_embedder": input_embedder}
    if sharded:
        md["sharded"] = True                                  # inner_loop then takes a GLOBAL batch and runs this rank's scenes (shard.sharded_inner_loop)
    return md


def pad_context_batch(clouds):
    """Context clouds of different sizes -> the padded batch the `context_counts` arguments take: clouds = a list of [M_b, C] GPU tensors
    (at least one point each, one C), returns (extract_0 [B, max M_b, C] fp32 with zeros behind every cloud, counts [B] int32 on the same
    device).  inner_loop((extract_0, extract_1, extra), ..., context_counts=counts) then scores scene b against clouds[b]."""
    clouds = list(clouds)
    if not clouds:
        raise RuntimeError("pad_context_batch: no clouds given")
    for i, c in enumerate(clouds):
        if not (torch.is_tensor(c) and c.is_cuda):
            raise RuntimeError(f"pad_context_batch: cloud {i} must be a tensor on a HIP device (there is no CPU path)")
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != clouds[0].shape[1] or c.device != clouds[0].device:
            raise RuntimeError(f"pad_context_batch: cloud {i} has shape {tuple(c.shape)} on {c.device}: every cloud must be [M_b, C] with M_b >= 1, "
                               f"C = {clouds[0].shape[1] if clouds[0].dim() == 2 else '?'} and on {clouds[0].device}")
    counts = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=clouds[0].device)
    extract_0 = torch.zeros(len(clouds), max(c.shape[0] for c in clouds), clouds[0].shape[1], dtype=torch.float32, device=clouds[0].device)
    for b, c in enumerate(clouds):
        extract_0[b, :c.shape[0]] = c
    return extract_0, counts


def pad_target_batch(clouds):
    """Target clouds of different sizes -> the padded batch the `target_counts` argument of inner_loop takes: clouds = a list of [N_b, C] GPU
    tensors (at least one point each, one C), returns (extract_1 [B, max N_b, C] fp32 with zeros behind every cloud, counts [B] int32 on the same
    device).  inner_loop((extract_0, extract_1, extra), ..., target_counts=counts) then scores the points of clouds[b] in scene b."""
    clouds = list(clouds)
    if not clouds:
        raise RuntimeError("pad_target_batch: no clouds given")
    for i, c in enumerate(clouds):
        if not (torch.is_tensor(c) and c.is_cuda):
            raise RuntimeError(f"pad_target_batch: cloud {i} must be a tensor on a HIP device (there is no CPU path)")
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != clouds[0].shape[1] or c.device != clouds[0].device:
            raise RuntimeError(f"pad_target_batch: cloud {i} has shape {tuple(c.shape)} on {c.device}: every cloud must be [N_b, C] with N_b >= 1, "
                               f"C = {clouds[0].shape[1] if clouds[0].dim() == 2 else '?'} and on {clouds[0].device}")
    counts = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=clouds[0].device)
    extract_1 = torch.zeros(len(clouds), max(c.shape[0] for c in clouds), clouds[0].shape[1], dtype=torch.float32, device=clouds[0].device)
    for b, c in enumerate(clouds):
        extract_1[b, :c.shape[0]] = c
    return extract_1, counts


def _check_target_counts(what, target_counts, batch, models_dict):
    """What `target_counts` cannot be combined with, and the tensor itself, before an embedder or the library runs.  Returns the counts as an
    int32 device tensor [B]."""
    from . import engine as _engine
    flow, embedder = models_dict["flow"], models_dict["input_embedder"]
    if flow.training or embedder.training:
        raise RuntimeError(f"{what}: target_counts is eval-mode only (train-mode statistics couple the rows of a batch, pad rows included): "
                           "initialize_flow(mode='test') or .eval() on the flow and the embedder")
    if models_dict.get("sharded"):
        raise RuntimeError(f"{what}: target_counts is not supported with a sharded models_dict (config['data_parallel']): the scene split does not "
                           "carry the counts -- give every rank its own scenes and counts through an unsharded models_dict")
    extract_1 = batch[1]
    if not (torch.is_tensor(extract_1) and extract_1.is_cuda):
        raise RuntimeError("flowcompare_amd: tensors must live on a HIP device (there is no CPU path)")
    return _engine._context_counts_range(target_counts, extract_1.shape[0], extract_1.shape[1], extract_1.device, "target_counts", side="target")[0]


def _check_context_counts(what, context_counts, batch, models_dict, config):
    """What `context_counts` cannot be combined with, and the tensor itself (engine._context_counts), before an embedder or the library runs.
    Returns the counts as a Python list."""
    from . import engine as _engine
    flow, embedder = models_dict["flow"], models_dict["input_embedder"]
    if flow.training or embedder.training:
        raise RuntimeError(f"{what}: context_counts is eval-mode only (the training path has no per-scene context point counts): "
                           "initialize_flow(mode='test') or .eval() on the flow and the embedder")
    if config["global"]:
        raise RuntimeError(f"{what}: context_counts has no meaning with config['global'] (the global embedder pools a whole cloud into one vector: "
                           "embed clouds of different sizes one by one instead)")
    if models_dict.get("sharded"):
        raise RuntimeError(f"{what}: context_counts is not supported with a sharded models_dict (config['data_parallel']): the scene split does not "
                           "carry the counts -- give every rank its own scenes and counts through an unsharded models_dict")
    extract_0 = batch[0]
    if not (torch.is_tensor(extract_0) and extract_0.is_cuda):
        raise RuntimeError("flowcompare_amd: tensors must live on a HIP device (there is no CPU path)")
    return _engine._context_counts(context_counts, extract_0.shape[0], extract_0.shape[1], extract_0.device).tolist()


def _embed_batch(batch, models_dict, config, context_counts=None, what="inner_loop"):
    """batch = (extract_0, extract_1, extra_context) -> (extract_1, emb, extra_context) as Flow.log_prob takes them: both clouds sliced to
    input_dim, the extra context repeated over config['sample_size'] points (einops.repeat 'b c -> b n c' in the reference), extract_0
    embedded and a global embedding repeated over the target points.
    context_counts ([B] integer GPU tensor): scene b's context cloud is extract_0[b, :count_b], the rows behind it are padding.  In eval mode
    an embedder row depends on its own scene only.  A count-aware embedder (the DGCNN modules, `count_aware` True) takes the padded batch
    and the counts in ONE call (its forward's context_counts): scene b gets the bytes it gets alone, pad rows of the
    embedding are exact zeros.  The PAConv module has the same path but is not count-aware by default: it is once
    `embedder.count_aware = True` is set on the instance.  Any other embedder (PAConv as shipped, or count_aware = False) embeds the scenes
    in groups of equal count on the unpadded clouds -- groups in ascending order of count, scene order kept inside a group -- with the
    embedder as it is and written into a zero-initialised [B, M, E]: one embedder call per DISTINCT count.  DGCNN needs
    count >= n_neighbors and PAConv count >= 256 either way.  The flow, more than 95 % of a step, runs once on the padded batch."""
    extract_0, extract_1, extra_context = batch
    Din = config["input_dim"]
    if context_counts is not None:
        counts = _check_context_counts(what, context_counts, batch, models_dict, config)
    extract_0, extract_1 = extract_0[:, :, :Din], extract_1[:, :, :Din]
    if extra_context is not None:
        extra_context = extra_context[:, None, :].expand(-1, config["sample_size"], -1)
    if context_counts is not None:
        embedder = models_dict["input_embedder"]
        if getattr(embedder, "count_aware", False):
            return extract_1, embedder(extract_0, context_counts=context_counts, count_range=(min(counts), max(counts))), extra_context
        emb = None
        for c in sorted(set(counts)):
            idx = torch.tensor([b for b, cb in enumerate(counts) if cb == c], dtype=torch.long, device=extract_0.device)
            part = models_dict["input_embedder"](extract_0.index_select(0, idx)[:, :c].contiguous())
            if emb is None:
                emb = torch.zeros(extract_0.shape[0], extract_0.shape[1], part.shape[-1], dtype=part.dtype, device=part.device)
            emb[idx, :c] = part
        return extract_1, emb, extra_context
    emb = models_dict["input_embedder"](extract_0)
    if config["global"]:
        emb = emb[:, None, :].expand(-1, extract_1.shape[1], -1)
    return extract_1, emb, extra_context


def inner_loop(batch, models_dict, config, eps=None, context_counts=None, target_counts=None):
    """model_initialization.py:206-228.  `eps` (optional) pins the augmenter noise.
    context_counts (optional, eval mode): an integer GPU tensor [B] -- scene b's context is extract_0[b, :count_b] (pad_context_batch builds
    such a batch from clouds of different sizes); a count-aware embedder (DGCNN; PAConv with `count_aware = True` on the instance) takes the
    padded batch and the counts in one call, any other one is called per group of equal count (_embed_batch); one flow call on the padded batch.
    target_counts (optional, eval mode, not with a sharded models_dict): an integer GPU tensor [B] with 1 <= n_b <= N --
    scene b's target is extract_1[b, :n_b] (pad_target_batch builds such a batch).  In eval mode a target point's log-prob depends on that point,
    its context and its own noise only, so the flow runs once on the padded batch: rows >= n_b of extract_1 are replaced by zeros first (whatever
    the caller's pad rows hold, it does not reach the flow or its range flag), log_prob[b, n_b:] comes back NaN (not evaluated), and loss / bpd are
    taken over the real slots only.  Goes with context_counts or without."""
    if target_counts is not None:
        counts_1 = _check_target_counts("inner_loop", target_counts, batch, models_dict)
        extract_0, extract_1, extra = batch
        real = torch.arange(extract_1.shape[1], device=extract_1.device)[None, :] < counts_1[:, None]
        with torch.no_grad():
            padded = (extract_0, torch.where(real[:, :, None], extract_1, extract_1.new_zeros(())), extra)
            _, log_prob, _ = inner_loop(padded, models_dict, config, eps=eps, context_counts=context_counts)
            loss = -log_prob[real].mean()
            bpd = loss * math.log2(math.exp(1)) / config["input_dim"]
            log_prob = torch.where(real, log_prob, log_prob.new_full((), float("nan")))
        return loss, log_prob, bpd
    if context_counts is not None:
        extract_1, emb, extra_context = _embed_batch(batch, models_dict, config, context_counts, "inner_loop")
        with torch.no_grad():
            log_prob = models_dict["flow"].log_prob(extract_1, context=emb, extra_context=extra_context, eps=eps, context_counts=context_counts)
            loss = -log_prob.mean()
            bpd = loss * math.log2(math.exp(1)) / config["input_dim"]
        return loss, log_prob, bpd
    if models_dict.get("sharded") and not models_dict.get("_in_shard"):
        # config['data_parallel']: `batch` is the GLOBAL batch, every rank runs its own scenes; returns (global loss, LOCAL log_prob, global bpd)
        from . import shard
        models_dict["_in_shard"] = True
        try:
            return shard.sharded_inner_loop(batch, models_dict, config, eps=eps)
        finally:
            models_dict["_in_shard"] = False
    extract_1, emb, extra_context = _embed_batch(batch, models_dict, config)
    log_prob = models_dict["flow"].log_prob(extract_1, context=emb, extra_context=extra_context, eps=eps)
    loss = -log_prob.mean()
    with torch.no_grad():
        bpd = loss * math.log2(math.exp(1)) / config["input_dim"]
    return loss, log_prob, bpd


def attention_weights(batch, models_dict, config, layers=("aug",), points=None, eps=None, return_log_prob=False, context_counts=None):
    """The attention maps visualize_attention.py colours the context cloud with (there: forward hooks on AttentionMine,
    models/perceiver.py:108-115), from the same pass as inner_loop: batch = (extract_0, extract_1, extra_context) is sliced, embedded and
    expanded exactly as inner_loop does.  layers: "aug" (the augmenter's attention) or 0-based flow-layer indices -- the reference
    script's three maps are layers=("aug", 50, 110); points: None (every target point) or integer indices [P] / [B, P] into extract_1.
    Returns a list of [B, P, M] tensors in the order of `layers` (row p: the weights of target point points[p] over the M context
    points, summing to 1), or (weights, log_prob) with return_log_prob.  The batch is taken as given: no scene sharding under
    config['data_parallel'] (every rank computes the scenes it is handed).  A full map is 4 B N M bytes per layer.
    context_counts as in inner_loop: scene b's rows hold its weights over its first count_b context points and exact zeros beyond."""
    extract_1, emb, extra_context = _embed_batch(batch, models_dict, config, context_counts, "attention_weights")
    return models_dict["flow"].attention_weights(extract_1, context=emb, extra_context=extra_context, layers=layers, points=points, eps=eps,
                                                 return_log_prob=return_log_prob, context_counts=context_counts)


def attention_mass(batch, models_dict, config, layers=("aug",), weights=None, eps=None, return_log_prob=False, context_counts=None):
    """Attention mass per context point, from the same pass as inner_loop (batch = (extract_0, extract_1, extra_context), sliced,
    embedded and expanded exactly as inner_loop does): mass[b, j] = sum_p weights[b, p] * w[b, p, j] with w the cross-attention softmax
    rows of attention_weights -- which points of the context cloud the target cloud (weights None = ones), its change score or a 0/1
    subset of its points relied on.  layers: "aug", 0-based flow-layer indices, or the string "all" (every attention of the flow in call
    order: flow.attention_layers()); weights: None or a GPU tensor [N] / [B, N], float or bool, finite -- a wrong shape, a non-finite
    value or a CPU tensor raises before the library is called.  Returns a list of [B, M] fp32 tensors in the order of `layers`, or
    (masses, log_prob) with return_log_prob.  No [B, N, M] map is formed (4 B M bytes per layer against 4 B N M), and the bytes are
    the same on every run.  The batch is taken as given: no scene sharding under config['data_parallel'].
    context_counts as in inner_loop: scene b's row holds the mass on its first count_b context points and exact zeros beyond."""
    from . import engine as _engine
    extract_0, extract_1, _ = batch
    if not (extract_0.is_cuda and extract_1.is_cuda):
        raise RuntimeError("flowcompare_amd: tensors must live on a HIP device (there is no CPU path)")
    _engine._row_weights(weights, extract_1.shape[0], extract_1.shape[1], extract_1.device)      # (refused here, before the embedder runs)
    extract_1, emb, extra_context = _embed_batch(batch, models_dict, config, context_counts, "attention_mass")
    return models_dict["flow"].attention_mass(extract_1, context=emb, extra_context=extra_context, layers=layers, weights=weights, eps=eps,
                                              return_log_prob=return_log_prob, context_counts=context_counts)


def _scene_min_context(what, min_context, models_dict, config):
    """min_context of the scene-level functions, checked before anything is staged: staging._min_context's rule, and eval mode, since every
    inner_loop call will carry `context_counts`."""
    from . import staging
    min_context = staging._min_context(what, min_context, config["n_samples_context"])
    if min_context is not None and (models_dict["flow"].training or models_dict["input_embedder"].training):
        raise RuntimeError(f"{what}: min_context is eval-mode only (it stages per-voxel context_counts, which the training path does not take): "
                           "initialize_flow(mode='test') or .eval() on the flow and the embedder")
    return min_context


def _scene_min_target(what, min_target, models_dict, config):
    """min_target of the scene-level functions, checked before anything is staged: an integer in [2, sample_size], and eval mode, since every
    inner_loop call will carry `target_counts`."""
    from . import staging
    min_target = staging._min_target(what, min_target, config["sample_size"], 2,
                                     " (a voxel's threshold is mean - multiple * std of its (0 | 0) baseline, and the unbiased std needs two values)")
    if min_target is not None and (models_dict["flow"].training or models_dict["input_embedder"].training):
        raise RuntimeError(f"{what}: min_target is eval-mode only (it stages per-voxel target_counts, which the training path does not take): "
                           "initialize_flow(mode='test') or .eval() on the flow and the embedder")
    if min_target is not None and models_dict.get("sharded"):
        raise RuntimeError(f"{what}: min_target is not supported with a sharded models_dict (config['data_parallel']): the scene split does not "
                           "carry the counts")
    return min_target


def dense_log_prob(st, dense, models_dict, config, blocks_per_batch=16, eps=None):
    """Log-probs of ALL members of the staged voxels against their voxel's staged context: st = the SceneStage (context st.extract_0,
    st.extra_context), dense = staging.stage_dense(...) of the same voxels.  In eval mode a target point's log-likelihood depends on
    that point, the context and the point's own augmenter noise only, so any member can be scored, not just
    the FPS sample.  The embedder runs once per staged voxel (chunks of blocks_per_batch voxels); every batch of blocks_per_batch blocks
    is one flow.log_prob with the blocks' voxels' embeddings / extra context gathered by index_select and expanded over the block as
    inner_loop does.  eps: None draws per batch as inner_loop does; otherwise one tensor [total, width_i] per noise site of the flow
    (flow.noise_shapes) in CSR row order -- pad slots get zeros.  Returns flat [total] log-probs in CSR order (dense.offsets /
    dense.rows); pad slots are dropped.  Eval mode, under torch.no_grad(); the batch is taken as given under config['data_parallel'].
    A SceneStage staged with min_context (st.context_counts set) is honoured: every chunk of voxels is embedded through
    _embed_batch with its counts (a DGCNN embedder: one call per chunk), and every flow.log_prob gets its blocks' counts, gathered like the embeddings."""
    if not (torch.is_tensor(st.extract_0) and st.extract_0.is_cuda and torch.is_tensor(dense.blocks) and dense.blocks.is_cuda):
        raise RuntimeError("dense_log_prob: expects a SceneStage and a DenseStage on the GPU (flowcompare_amd has no CPU fallback)")
    flow, embedder = models_dict["flow"], models_dict["input_embedder"]
    if flow.training or embedder.training:
        raise RuntimeError("dense_log_prob is eval-mode only (train-mode statistics couple the rows of a batch): call .eval() first")
    blocks_per_batch = int(blocks_per_batch)
    if blocks_per_batch < 1:
        raise RuntimeError("dense_log_prob: blocks_per_batch must be at least 1")
    K1, (n_blocks, block), Din = st.extract_0.shape[0], dense.index.shape, config["input_dim"]
    if dense.offsets.numel() != K1 + 1:
        raise RuntimeError(f"dense_log_prob: the DenseStage lists {dense.offsets.numel() - 1} voxels, the SceneStage staged {K1}")
    member = dense.index.reshape(-1) >= 0
    if eps is not None:
        widths = [s[2] for s in flow.noise_shapes(1, 1)]
        total = dense.rows.numel()
        if len(eps) != len(widths) or any(not e.is_cuda or tuple(e.shape) != (total, w) for e, w in zip(eps, widths)):
            raise RuntimeError(f"dense_log_prob: eps must be one GPU tensor [{total}, width] per noise site, widths {widths}")
        csr_pos = (torch.cumsum(member, 0) - 1).clamp_(min=0)                     # CSR position of every slot (pads: any valid row, zeroed below)
    out = torch.empty(n_blocks, block, dtype=torch.float32, device=dense.blocks.device)
    counts = getattr(st, "context_counts", None)
    with torch.no_grad():
        if n_blocks and counts is not None:
            emb = torch.cat([_embed_batch((st.extract_0[a:a + blocks_per_batch], st.extract_1[a:a + blocks_per_batch], None), models_dict, config,
                                          counts[a:a + blocks_per_batch], "dense_log_prob")[1] for a in range(0, K1, blocks_per_batch)])
        elif n_blocks:
            emb = torch.cat([embedder(st.extract_0[a:a + blocks_per_batch, :, :Din]) for a in range(0, K1, blocks_per_batch)])
        for a in range(0, n_blocks, blocks_per_batch):
            b = min(a + blocks_per_batch, n_blocks)
            voxel = dense.block_voxel[a:b].long()
            context = emb.index_select(0, voxel)
            if config["global"]:
                context = context[:, None, :].expand(-1, block, -1)
            extra = None
            if config.get("using_extra_context"):
                extra = st.extra_context.index_select(0, voxel)[:, None, :].expand(-1, block, -1)
            noise = None
            if eps is not None:
                sl = slice(a * block, b * block)
                noise = [torch.where(member[sl, None], e.index_select(0, csr_pos[sl]), e.new_zeros(())).reshape(b - a, block, -1) for e in eps]
            if counts is None:
                out[a:b] = flow.log_prob(dense.blocks[a:b, :, :Din], context=context, extra_context=extra, eps=noise)
            else:
                out[a:b] = flow.log_prob(dense.blocks[a:b, :, :Din], context=context, extra_context=extra, eps=noise,
                                         context_counts=counts.index_select(0, voxel))
    return out.reshape(-1)[member]


def scene_change(cloud_0, cloud_1, models_dict, config, centers, ground_height=None, multiple=5.4, hard_cutoff=None, voxels_per_batch=16,
                 final_voxel_size=None, context_voxel_size=None, dense=False, block=None, min_context=None, min_target=None):
    """test_flow.py:151-166 for a whole scene, one direction: the change of cloud_1 [P1, C] given cloud_0 [P0, C] at the voxel centres
    `centers` [K, 3].  Sample counts are config['sample_size'] / config['n_samples_context'] as the reference's loader takes them
    (test_flow.py:141-143); the box sizes default to the config's 'final_voxel_size' / 'context_voxel_size'.  Evaluated are the centres
    valid for BOTH stagings needed, (1 | 0) = context of cloud 0, target of cloud 1 and (0 | 0) = context and target of cloud 0, so that
    row k of both log-prob tensors is the same voxel.  inner_loop runs on chunks of `voxels_per_batch` voxels; like the reference the
    (0 | 0) batch takes the extra context of the (1 | 0) batch.  log_prob_to_change acts per chunk: its clamp_infs takes the minimum
    over the tensor it is given, i.e. per chunk here exactly as per loader batch in the reference.  Returns (change [P1], the (1 | 0)
    SceneStage with `voxel` / counts referring to `centers`): NaN where a point was not evaluated, the larger value where two voxels
    share a sampled point.  The augmenter noise is drawn as inner_loop draws it: seed torch's device generator for a reproducible map.

    dense=True scores EVERY point of cloud_1 inside an evaluated voxel, not only the FPS sample.  Validity,
    both stagings, the context, the normalisation, the extra context and the sampled (0 | 0) baseline (chunks of voxels_per_batch) stay
    as above; (1 | 0) is dense_log_prob over all members of the final box in blocks of `block` rows (default config['sample_size'],
    voxels_per_batch blocks per flow call), and ONE log_prob_to_change_ragged call covers the scene: min / max scaling over all of a
    voxel's members, threshold from its sampled (0 | 0) row.  Unlike the sampled mode, whose clamp_infs acts per chunk, the dense mode's
    clamp_infs acts over the whole scene's tensor.  Every point inside an evaluated voxel comes back finite (the larger value where boxes
    share a face), points of voxels that fail the validity mask stay NaN, and the returned SceneStage carries the DenseStage as `.dense`.

    min_context (an integer in [1, n_samples_context], eval mode) also evaluates voxels whose context box holds fewer
    than n_samples_context points: the validity mask becomes (c0_ctx >= min_context) & (c1_fin >= N) & (c0_fin >= N), both stagings are made
    with stage_scene's min_context (they share the context boxes, so the counts), and every inner_loop / dense_log_prob call passes its
    voxels' counts as `context_counts`; the returned SceneStage carries them as `.context_counts`.  A count-aware embedder (DGCNN; PAConv with
    `count_aware = True` on the instance) then runs once per chunk, any other one once per DISTINCT count of a chunk (_embed_batch), and its own
    minimum applies (DGCNN: n_neighbors points, PAConv: 256).

    min_target (an integer in [2, sample_size], eval mode) also evaluates voxels whose FINAL boxes hold fewer than
    sample_size points -- where something was removed, appeared in a nearly empty place, or the scene ends: the validity mask becomes
    (context rule) & (c1_fin >= min_target) & (c0_fin >= min_target), both stagings are made with stage_scene's min_target and carry their own
    `target_counts` (the (1 | 0) target is cloud 1, the (0 | 0) target cloud 0).  Sampled mode: every inner_loop gets its staging's counts as
    `target_counts`, log_prob_to_change_counts acts per chunk on the real slots, and the change is scattered through index_1 >= 0 only.  Dense mode:
    a sparse voxel's members are all picked, so its single block is its sample; log_prob_to_change_ragged takes the (0 | 0) counts as base_counts.
    2 is the lowest value because a voxel's threshold needs the unbiased std of its baseline.  Goes with min_context or without."""
    from . import change as change_ops
    from . import staging
    fin = config.get("final_voxel_size") if final_voxel_size is None else final_voxel_size
    ctx = config.get("context_voxel_size") if context_voxel_size is None else context_voxel_size
    if fin is None or ctx is None:
        raise RuntimeError("scene_change: final_voxel_size / context_voxel_size are neither given nor in the config")
    if config.get("using_extra_context") and ground_height is None:
        raise RuntimeError("scene_change: this config uses the extra z-value context and needs ground_height")
    N, M = config["sample_size"], config["n_samples_context"]
    min_context = _scene_min_context("scene_change", min_context, models_dict, config)
    min_target = _scene_min_target("scene_change", min_target, models_dict, config)
    c0_ctx, c1_fin, c0_fin = (staging.voxel_counts(cloud_0, centers, ctx), staging.voxel_counts(cloud_1, centers, fin),
                              staging.voxel_counts(cloud_0, centers, fin))
    n_min = N if min_target is None else min_target
    both = torch.nonzero((c0_ctx >= (M if min_context is None else min_context)) & (c1_fin >= n_min) & (c0_fin >= n_min)).flatten()
    sel = centers[both].contiguous()
    st10 = staging.stage_scene(cloud_0, cloud_1, sel, fin, ctx, N, M, ground_height, min_context=min_context, min_target=min_target)
    st00 = staging.stage_scene(cloud_0, cloud_0, sel, fin, ctx, N, M, ground_height, min_context=min_context, min_target=min_target)
    assert st10.voxel.numel() == st00.voxel.numel() == both.numel()
    counts = st10.context_counts                                  # None without min_context; st00's are the same (same context boxes)
    t10, t00 = st10.target_counts, st00.target_counts             # None without min_target; each staging has its own (different target clouds)
    out = torch.full((cloud_1.shape[0],), float("nan"), dtype=torch.float32, device=cloud_1.device)
    if dense:
        st10.dense = staging.stage_dense(cloud_1, st10, fin, sel, N if block is None else block)
        if both.numel():
            lp_1_0 = dense_log_prob(st10, st10.dense, models_dict, config, blocks_per_batch=voxels_per_batch)
            lp_0_0 = []
            with torch.no_grad():
                for a in range(0, both.numel(), voxels_per_batch):
                    sl = slice(a, a + voxels_per_batch)
                    extra = st10.extra_context[sl] if config.get("using_extra_context") else None
                    lp_0_0.append(inner_loop((st00.extract_0[sl], st00.extract_1[sl], extra), models_dict, config,
                                             context_counts=None if counts is None else counts[sl],
                                             target_counts=None if t00 is None else t00[sl])[1])
            change = change_ops.log_prob_to_change_ragged(lp_1_0, st10.dense.offsets, torch.cat(lp_0_0), multiple, hard_cutoff, base_counts=t00)
            out.scatter_reduce_(0, st10.dense.rows, change, "amax", include_self=False)
        st10.voxel, st10.count_0, st10.count_1 = both, c0_ctx, c1_fin
        return out, st10
    chunks = []
    with torch.no_grad():
        for a in range(0, both.numel(), voxels_per_batch):
            sl = slice(a, a + voxels_per_batch)
            extra = st10.extra_context[sl] if config.get("using_extra_context") else None
            cnt = None if counts is None else counts[sl]
            n10, n00 = (None, None) if min_target is None else (t10[sl], t00[sl])
            _, lp_1_0, _ = inner_loop((st10.extract_0[sl], st10.extract_1[sl], extra), models_dict, config, context_counts=cnt, target_counts=n10)
            _, lp_0_0, _ = inner_loop((st00.extract_0[sl], st00.extract_1[sl], extra), models_dict, config, context_counts=cnt, target_counts=n00)
            chunks.append(change_ops.log_prob_to_change(lp_1_0, lp_0_0, multiple, hard_cutoff) if min_target is None else
                          change_ops.log_prob_to_change_counts(lp_1_0, n10, lp_0_0, n00, multiple, hard_cutoff))
    if chunks:
        rows, vals = st10.index_1.reshape(-1), torch.cat(chunks).reshape(-1)
        if min_target is not None:                                # pad slots of sparse voxels: index -1, change NaN -- they name no row
            real = torch.nonzero(rows >= 0).flatten()
            rows, vals = rows.index_select(0, real), vals.index_select(0, real)
        out.scatter_reduce_(0, rows, vals, "amax", include_self=False)
    st10.voxel, st10.count_0, st10.count_1 = both, c0_ctx, c1_fin
    return out, st10


def scene_context_attribution(cloud_0, cloud_1, models_dict, config, centers, layers=("aug",), ground_height=None, multiple=5.4, hard_cutoff=None,
                              voxels_per_batch=16, weight="change", min_context=None, min_target=None):
    """Which points of the OLD scan the change map relied on: the sampled mode of scene_change (same validity rule, stagings, sample
    counts, chunks of `voxels_per_batch` voxels, log_prob_to_change per chunk) plus, per chunk, attention_mass on the (1 | 0) batch with
    weights = that chunk's change (weight="change") or ones (weight="uniform").  Per chunk ONE set of augmenter / CIF noise is drawn from
    flow.noise_shapes and used by all three passes, so the mass belongs to the very pass that scored the change.  (scene_change lets
    every inner_loop draw its own noise: the change here equals scene_change's bit for bit under the same seed for a flow that draws
    none, and is another sample of the same quantity otherwise.)  layers as in attention_mass ("all" included).
    Returns (mass_0 [len(layers), P0], change_1 [P1], the (1 | 0) SceneStage): mass_0[i, r] = layer i's mass on row r of cloud_0, scattered
    through st10.index_0 -- NaN where no evaluated voxel sampled the row as context, the larger value where two voxels share it (the
    rule scene_change applies to shared points; deterministic); change_1 as scene_change returns it.
    min_context as in scene_change: every pass of a chunk gets the chunk's counts, and mass is scattered only through index_0 >= 0 -- the pad
    slots of a sparse voxel hold exact zeros and reach no row of cloud_0.
    min_target as in scene_change's sampled mode: target pad slots get weight 0 in attention_mass -- weight="change": the change with its NaN pads
    replaced by 0, weight="uniform": the 0/1 mask of real slots -- and the change is scattered through index_1 >= 0 only."""
    from . import change as change_ops
    from . import staging
    if weight not in ("change", "uniform"):
        raise RuntimeError(f"scene_context_attribution: weight must be \"change\" or \"uniform\", got {weight!r}")
    fin, ctx = config.get("final_voxel_size"), config.get("context_voxel_size")
    if fin is None or ctx is None:
        raise RuntimeError("scene_context_attribution: final_voxel_size / context_voxel_size are not in the config")
    if config.get("using_extra_context") and ground_height is None:
        raise RuntimeError("scene_context_attribution: this config uses the extra z-value context and needs ground_height")
    flow = models_dict["flow"]
    if isinstance(layers, str):
        layers = flow.attention_layers() if layers == "all" else (layers,)
    layers = list(layers)
    N, M = config["sample_size"], config["n_samples_context"]
    min_context = _scene_min_context("scene_context_attribution", min_context, models_dict, config)
    min_target = _scene_min_target("scene_context_attribution", min_target, models_dict, config)
    c0_ctx, c1_fin, c0_fin = (staging.voxel_counts(cloud_0, centers, ctx), staging.voxel_counts(cloud_1, centers, fin),
                              staging.voxel_counts(cloud_0, centers, fin))
    n_min = N if min_target is None else min_target
    both = torch.nonzero((c0_ctx >= (M if min_context is None else min_context)) & (c1_fin >= n_min) & (c0_fin >= n_min)).flatten()
    sel = centers[both].contiguous()
    st10 = staging.stage_scene(cloud_0, cloud_1, sel, fin, ctx, N, M, ground_height, min_context=min_context, min_target=min_target)
    st00 = staging.stage_scene(cloud_0, cloud_0, sel, fin, ctx, N, M, ground_height, min_context=min_context, min_target=min_target)
    assert st10.voxel.numel() == st00.voxel.numel() == both.numel()
    counts = st10.context_counts
    t10, t00 = st10.target_counts, st00.target_counts
    change_1 = torch.full((cloud_1.shape[0],), float("nan"), dtype=torch.float32, device=cloud_1.device)
    mass_0 = torch.full((len(layers), cloud_0.shape[0]), float("nan"), dtype=torch.float32, device=cloud_0.device)
    chunks, masses = [], []
    with torch.no_grad():
        for a in range(0, both.numel(), voxels_per_batch):
            sl = slice(a, a + voxels_per_batch)
            extra = st10.extra_context[sl] if config.get("using_extra_context") else None
            batch_10 = (st10.extract_0[sl], st10.extract_1[sl], extra)
            eps = [torch.randn(s, device=cloud_1.device, dtype=torch.float32) for s in flow.noise_shapes(st10.extract_1[sl].shape[0], N)]
            cnt = None if counts is None else counts[sl]
            n10, n00 = (None, None) if min_target is None else (t10[sl], t00[sl])
            _, lp_1_0, _ = inner_loop(batch_10, models_dict, config, eps=eps, context_counts=cnt, target_counts=n10)
            _, lp_0_0, _ = inner_loop((st00.extract_0[sl], st00.extract_1[sl], extra), models_dict, config, eps=eps, context_counts=cnt, target_counts=n00)
            if min_target is None:
                change = change_ops.log_prob_to_change(lp_1_0, lp_0_0, multiple, hard_cutoff)
                w = change if weight == "change" else None
            else:                                                 # weight 0 on the target pad slots, whose change is NaN
                change = change_ops.log_prob_to_change_counts(lp_1_0, n10, lp_0_0, n00, multiple, hard_cutoff)
                w = change.nan_to_num(nan=0.0) if weight == "change" else (st10.index_1[sl] >= 0).to(torch.float32)
            chunks.append(change)
            masses.append(torch.stack(attention_mass(batch_10, models_dict, config, layers=layers, weights=w, eps=eps, context_counts=cnt)))
    if chunks:
        rows_1, vals_1 = st10.index_1.reshape(-1), torch.cat(chunks).reshape(-1)
        if min_target is not None:                                # target pad slots: index -1, change NaN -- they name no row
            real_1 = torch.nonzero(rows_1 >= 0).flatten()
            rows_1, vals_1 = rows_1.index_select(0, real_1), vals_1.index_select(0, real_1)
        change_1.scatter_reduce_(0, rows_1, vals_1, "amax", include_self=False)
        rows, vals = st10.index_0.reshape(-1), torch.cat(masses, dim=1).reshape(len(layers), -1)
        if counts is not None:                                    # pad slots of sparse voxels: index -1, mass 0.0 -- they name no row
            real = torch.nonzero(rows >= 0).flatten()
            rows, vals = rows.index_select(0, real), vals.index_select(1, real)
        mass_0.scatter_reduce_(1, rows.reshape(1, -1).expand(len(layers), -1), vals, "amax", include_self=False)
    st10.voxel, st10.count_0, st10.count_1 = both, c0_ctx, c1_fin
    return mass_0, change_1, st10


def make_sample(n_points, extract_0, models_dict, config, sample_distrib=None, extra_context=None):
    """model_initialization.py:231-245."""
    extract_0 = extract_0[:, :, :config["input_dim"]]
    emb = models_dict["input_embedder"](extract_0)
    if extra_context is not None:
        extra_context = extra_context[:, None, :].expand(-1, n_points, -1)
    if config["global"]:
        emb = emb[:, None, :].expand(-1, n_points, -1)
    x = models_dict["flow"].sample(num_samples=1, n_points=n_points, context=emb, sample_distrib=sample_distrib,
                                   extra_context=extra_context).squeeze()
    return x
