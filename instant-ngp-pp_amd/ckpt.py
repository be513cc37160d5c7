"""Checkpoint helpers with the reference's layout (utils.py:7-42): Lightning-style
`{'state_dict': {'model.<key>': tensor, ...}}` files, the model's keys under a `model.` prefix,
tcnn modules as flat `*.params` vectors.  Loading uses weights_only=True (no unpickling of code)."""
import torch


def extract_model_state_dict(ckpt_path, model_name='model', prefixes_to_ignore=()):
    checkpoint = torch.load(ckpt_path, map_location='cpu', weights_only=True)
    if 'state_dict' in checkpoint:  # pytorch-lightning checkpoint
        checkpoint = checkpoint['state_dict']
    out = {}
    for k, v in checkpoint.items():
        if not k.startswith(model_name):
            continue
        k = k[len(model_name) + 1:]
        if any(k.startswith(p) for p in prefixes_to_ignore):
            continue
        out[k] = v
    return out


def load_ckpt(model, ckpt_path, model_name='model', prefixes_to_ignore=()):
    """in-place update of `model` from a (slim) checkpoint; parameter storage (e.g. the trainer's
    flat buffer views) is preserved because values are copied, not rebound.  Strict like the reference's
    load_state_dict (utils.py:24-29): unknown keys and shape mismatches raise.  With a sharded-optimizer
    trainer use NGPTrainer.load_ckpt (it refreshes the optimizer's master slices afterwards)."""
    if not ckpt_path:
        return
    state = extract_model_state_dict(ckpt_path, model_name, prefixes_to_ignore)
    own = model.state_dict()
    missing = [k for k in state if k not in own]
    if missing:
        raise KeyError(f"checkpoint keys not in the model: {missing[:5]}")
    bad = [(k, tuple(v.shape), tuple(own[k].shape)) for k, v in state.items() if tuple(v.shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError("size mismatch for " + ", ".join(f"{k}: checkpoint {a} vs model {b}" for k, a, b in bad[:5]))
    with torch.no_grad():
        for k, v in state.items():
            own[k].copy_(v.to(own[k].device))


def save_ckpt(model, path, extra=None, msk_model=None, embedding_a=None, pose_refiner=None):
    """writes {'state_dict': {'model.<key>': ...}} like Lightning's ModelCheckpoint(save_weights_only); the transient
    mask model of the embed_msk recipe goes beside it under 'msk_model.<key>' (train.py:112-113, 236) and the appearance
    table of the embed_a recipe (an nn.Embedding, or a FrameEmbedding's) as 'embedding_a.weight' (train.py:104-108); the
    pose corrections of the optimize_ext recipe (a pose.PoseRefiner) as 'dR', 'dT' and 'poses' at the top level, the keys
    Lightning gives the reference's system (train.py:222-230) and slim_ckpt(save_poses=True) keeps"""
    sd = {f"model.{k}": v.detach().cpu() for k, v in model.state_dict().items()}
    if msk_model is not None:
        sd.update({f"msk_model.{k}": v.detach().cpu() for k, v in msk_model.state_dict().items()})
    if embedding_a is not None:    # (behind the mask model: the order in which train.py registers the three)
        embedding_a = getattr(embedding_a, "embedding_a", embedding_a)
        sd.update({f"embedding_a.{k}": v.detach().cpu().clone() for k, v in embedding_a.state_dict().items()})
    if pose_refiner is not None:
        sd.update({k: v.detach().cpu().clone() for k, v in pose_refiner.state_dict().items()})
    if extra:
        sd.update(extra)
    torch.save({'state_dict': sd}, path)


def load_poses(pose_refiner, ckpt_path):
    """in-place update of a pose.PoseRefiner from the top-level 'dR', 'dT' and 'poses' of a checkpoint (values are copied:
    a trainer's pose buffer stays bound); a checkpoint without them or with other shapes raises"""
    checkpoint = torch.load(ckpt_path, map_location='cpu', weights_only=True)
    checkpoint = checkpoint.get('state_dict', checkpoint)
    own = pose_refiner.state_dict()
    missing = [k for k in own if k not in checkpoint]
    if missing:
        raise KeyError(f"checkpoint has no pose keys {missing}")
    bad = [(k, tuple(checkpoint[k].shape), tuple(own[k].shape)) for k in own if tuple(checkpoint[k].shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError("size mismatch for " + ", ".join(f"{k}: checkpoint {a} vs refiner {b}" for k, a, b in bad))
    with torch.no_grad():
        for k in own:
            own[k].copy_(checkpoint[k].to(own[k].device))


def slim_ckpt(ckpt_path, save_poses=False):
    """drops what inference does not need (utils.py:32-42)"""
    ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=True)
    keys_to_pop = ['directions', 'model.density_grid', 'model.grid_coords']
    if not save_poses:
        keys_to_pop += ['poses']
    keys_to_pop += [k for k in ckpt['state_dict'] if k.startswith('val_lpips')]
    for k in keys_to_pop:
        ckpt['state_dict'].pop(k, None)
    return ckpt['state_dict']
