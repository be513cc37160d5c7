"""Per-image appearance codes (the reference's `embed_a` recipe: train.py:104-108, 238-244, utils.py:97-143).

  FrameEmbedding(embed_a_len, poses, ckpt_path=None)   the table (nn.Embedding(len(poses), embed_a_len) as `embedding_a`)
                                                       and its three read-outs: the code of an image index, of the
                                                       training pose nearest to a camera, or the mean of the two nearest
  RayCodes(weight, img_idxs)                           what a TRAINING render takes as embedding_a= instead of a
                                                       (n_rays, E) tensor: the table itself and the image of every ray

With RayCodes the field broadcasts the codes into rgb_net's input with one launch (ngp_embed_a_fwd, which also writes the
ones-padding) and sums their gradient per image with one launch (ngp_embed_a_bwd), straight into the trainer's flat
gradient when there is one.  A (n_rays, E) or (N, E) tensor keeps working as before (expanded with torch operations).
Test-time rendering takes a (1, E) tensor, as the reference does (train.py:153-154).
"""
import torch
from torch import nn

from .ckpt import load_ckpt


class FrameEmbedding(nn.Module):
    def __init__(self, embed_a_len, poses, ckpt_path=None):
        """poses (n_imgs, 3, 4) camera-to-world matrices of the training images; ckpt_path: a checkpoint that holds
        'embedding_a.weight' (ckpt.save_ckpt(..., embedding_a=))"""
        super().__init__()
        self.poses = poses
        embedding_a = nn.Embedding(len(poses), embed_a_len)
        if ckpt_path is not None:
            load_ckpt(embedding_a, ckpt_path, model_name='embedding_a', prefixes_to_ignore=['model', 'msk_model'])
        self.embedding_a = embedding_a

    def forward(self, x, mode='index'):
        """mode 'index': x an int or an integer tensor -> the codes of those images ((1, E) for an int);
        'nearest': x a (3, 4) pose -> (1, E), the code of the training camera closest to it;
        'mean': x a (3, 4) pose -> (1, E), the mean of the codes of the two closest training cameras"""
        if mode == 'index':
            return self.sample_index(x)
        if mode == 'nearest':
            return self.sample_nearest(x)
        if mode == 'mean':
            return self.sample_mean(x)
        raise ValueError('Invalid mode: {}'.format(mode))

    def _sq_dist(self, pose):
        centres = self.poses[:, :3, -1]
        return torch.sum((centres - pose[:3, -1].to(centres.device)) ** 2, dim=1)

    def sample_index(self, index):
        if not torch.is_tensor(index):
            index = torch.tensor([index])
        return self.embedding_a(index.to(self.embedding_a.weight.device))

    def sample_nearest(self, pose):
        index = torch.argmin(self._sq_dist(pose)).reshape(1)
        return self.embedding_a(index.to(self.embedding_a.weight.device))

    def sample_mean(self, pose):
        _, indices = torch.topk(-self._sq_dist(pose), 2)
        return torch.mean(self.embedding_a(indices.to(self.embedding_a.weight.device)), dim=0, keepdim=True)


class RayCodes:
    """embedding_a= of a training render: `weight` (n_imgs, E) float32, the embedding table (an nn.Embedding's weight, a
    Parameter, or any tensor), and `img_idxs` (n_rays) int64, the image every ray of the batch belongs to.  An index
    outside [0, n_imgs) gives that ray a zero code and no gradient.  render() binds the batch's rays_a
    (`for_batch`); the field then runs ngp_embed_a_fwd / ngp_embed_a_bwd."""

    __slots__ = ("weight", "img_idxs", "rays_a")

    def __init__(self, weight, img_idxs, rays_a=None):
        if isinstance(weight, nn.Embedding):
            weight = weight.weight
        if weight.dim() != 2 or weight.dtype != torch.float32:
            raise ValueError("weight must be a (n_imgs, E) float32 tensor")
        if not 1 <= weight.shape[1] <= 32:
            raise ValueError(f"codes of length {weight.shape[1]}: 1 to 32 are supported")
        img_idxs = torch.as_tensor(img_idxs)
        if img_idxs.dim() != 1 or img_idxs.dtype.is_floating_point:
            raise ValueError("img_idxs must be a 1-D integer tensor, one image index per ray")
        self.weight = weight
        self.img_idxs = img_idxs.to(device=weight.device, dtype=torch.int64).contiguous()
        self.rays_a = rays_a

    def for_batch(self, rays_a):
        """-> the same codes bound to the (n_rays, 3) sample segments of the batch"""
        if rays_a.shape[0] != self.img_idxs.shape[0]:
            raise ValueError(f"img_idxs names {self.img_idxs.shape[0]} rays, the batch has {rays_a.shape[0]}")
        return RayCodes(self.weight, self.img_idxs, rays_a)

    def expand(self):
        """the (N, E) per-sample codes through torch operations (the differentiable-normals route, which builds its
        input matrix with torch.cat); out-of-range indices give zero rows here as well"""
        if self.rays_a is None:
            raise ValueError("RayCodes is not bound to a ray batch: pass it to render(), which binds rays_a")
        n_imgs = self.weight.shape[0]
        ok = (self.img_idxs >= 0) & (self.img_idxs < n_imgs)
        per_ray = self.weight[self.img_idxs.clamp(0, n_imgs - 1)] * ok[:, None]
        return torch.repeat_interleave(per_ray[self.rays_a[:, 0]], self.rays_a[:, 2], 0)
