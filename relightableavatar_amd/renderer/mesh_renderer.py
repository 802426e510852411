"""Mesh extraction: lib/networks/renderer/mesh_renderer.py, Renderer.render(batch), on the device.

    volume      Engine.sdf_volume      :42-72   -sdf on the grid points the K-NN filter keeps, -10 elsewhere, padded by 10
    threshold   cfg.mesh_th, or alpha2sdf(cfg.mesh_th, beta) with cfg.mesh_th_to_sdf   :74-77 (data_utils.py:50-51)
    surface     Engine.marching_cubes  :80      then (verts - 10) * voxel_size[0] + bounds[0, 0]   :81-87
    component   Engine.largest_component   :92-93
    materials   albedo_network on the features of the vertices, for albedo AND roughness   :101-128
    weights     sample_blend_K_closest_points / sample_closest_points_on_surface   :132-137

Selected by make_renderer when cfg.vis_can_mesh / vis_tpose_mesh / vis_posed_mesh is set.  The grid comes from batch.pts when the batch
carries the reference's (B, x, y, z, 3) array, else from data_utils.mesh_grid_axes on the mode's bounds.  Reference quirks kept (DESIGN.md
section 6): voxel_size[0] scales all three axes; `roughness` is a second evaluation of the ALBEDO network.  Not kept: mcubes' vertex / face order and winding and trimesh.Trimesh's vertex merging (DESIGN.md
section 18); cfg.mesh_simp_face is refused.  Returned: verts float32, faces / parents int32, weights, joints, tjoints — numpy, as the
reference returns them — and albedo / roughness as device tensors.  Three blocking read-backs before the results are copied out (kept
points, vertex / face counts, component result); with cfg.mesh_th_to_sdf the network's beta is read to the host once, when the
renderer is made, not per frame.
"""
import math

import numpy as np
import torch

from .. import config, data_utils, mesh_utils
from ..base_utils import dotdict

PAD, FILL = 10, -10.0


def alpha2sdf(alpha, beta, dists=0.005):
    return beta * math.log(2 * beta * (-math.log(1 - alpha) / dists))


class Renderer:
    def __init__(self, net):
        self.net = net
        cfg = config.active_cfg()
        # a device parameter: read here, once, so that render() makes no fourth read-back
        self.beta = float(net.signed_distance_network.beta) if cfg.get('mesh_th_to_sdf', False) and hasattr(net, 'signed_distance_network') else None

    def mode(self, batch):
        cfg = config.active_cfg()
        latent = batch.meta.latent_index if 'meta' in batch and 'latent_index' in batch.meta else None
        if cfg.vis_can_mesh or (cfg.vis_tpose_mesh and latent is not None and int(torch.as_tensor(latent).reshape(-1)[0]) == -1):
            return 'canonical'
        if cfg.vis_posed_mesh:
            return 'posed'
        if cfg.vis_tpose_mesh:
            return 'tpose'
        raise NotImplementedError('mesh_renderer: none of cfg.vis_can_mesh, vis_tpose_mesh, vis_posed_mesh is set')

    @staticmethod
    def world_verts(batch):
        """batch.wverts, or the pose-space vertices moved to the world: ppts = (x - Th) @ R inverted"""
        if 'wverts' in batch:
            return batch.wverts
        return batch.pverts @ batch.R.transpose(-1, -2) + batch.Th.reshape(-1, 1, 3)

    def render(self, batch):
        cfg = config.active_cfg()
        mode = self.mode(batch)
        posed = cfg.vis_posed_mesh and not (cfg.vis_can_mesh or cfg.vis_tpose_mesh)       # which vertices and bounds: mesh_renderer.py:37-40, 82-85
        eng = self.net.set_frame(batch)
        dev = eng.device
        ref = (self.world_verts(batch) if posed else batch.tverts).to(dev).float()
        bounds = (batch.wbounds if posed else batch.tbounds).to(dev).float()
        if 'pts' in batch:
            pts = torch.as_tensor(batch.pts)
            axes = (pts[0, :, 0, 0, 0], pts[0, 0, :, 0, 1], pts[0, 0, 0, :, 2])
        else:
            axes = data_utils.mesh_grid_axes(bounds[0], cfg.voxel_size)
        volume = eng.sdf_volume(*axes, mode, cfg.dist_th, fill=FILL, pad=PAD, verts=ref[0])
        th = cfg.mesh_th
        if cfg.mesh_th_to_sdf and self.beta is not None:
            th = alpha2sdf(cfg.mesh_th, self.beta)
        verts, faces = eng.marching_cubes(volume, th)
        verts = (verts - PAD) * float(cfg.voxel_size[0]) + bounds[0, 0]
        verts, faces = eng.largest_component(verts, faces)
        ret = dotdict()
        if hasattr(self.net, 'albedo_network') and verts.shape[0]:
            if mode == 'posed':
                # inference_world_geometry + albedo_network is the network's full query: the albedo channels of its raw output.  (Not
                # ra_bigpose_transform: its matrix inverts the blended bone transform by transposition, as the reference's
                # world_to_bigpose_transform does, and so does not give the points the forward pass warps to)
                albedo = eng.forward(verts, None, cfg.dist_th)[:, 9:12].contiguous()
            else:
                feat = eng.canonical_features(verts) if mode == 'canonical' else eng.bigpose_features(verts)
                albedo, _ = eng.heads_forward(eng.heads_params(), feat)
            ret.albedo, ret.roughness = albedo, albedo.clone()      # :105-106, 112-113, 122-123: albedo_network for both
        weights = batch.weights.to(dev).float()
        if cfg.surface_blend_weight:
            weights, _ = mesh_utils.sample_closest_points_on_surface(verts[None], ref, batch.faces.to(dev), weights, engine=eng)
        else:
            weights, _ = mesh_utils.sample_blend_K_closest_points(verts[None], ref, weights, K=cfg.sample_vert_cnt)
        npy = lambda t: t.detach().cpu().numpy()
        for key, src in (('joints', 'joints' if posed else 'big_joints'), ('tjoints', 'tjoints')):
            if src in batch:
                ret[key] = npy(batch[src][0])
        if 'parents' in batch:
            ret.parents = npy(batch.parents[0]).astype(np.int32)
        ret.weights = npy(weights[0])
        ret.verts = npy(verts).astype(np.float32)
        ret.faces = npy(faces).astype(np.int32)
        return ret
