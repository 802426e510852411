"""Writing an extracted mesh to disk (lib/visualizers/mesh_visualizer.py).

    Visualizer.visualize(output, batch)     :14-36: `<name>.npz` with every array of `output`, `<name>.ply` with the mesh
    export_mesh(verts, faces, filename, subdivision)     lib/utils/data_utils.py:251-265 for .ply and .npz, without trimesh;
                                            subdivision=N runs N Loop steps on the device first (mesh_utils.loop_subdivision)

The file names follow the reference's rule: `can_mesh` for the canonical mesh (cfg.vis_can_mesh, or latent index -1 of a tracked
T-pose mesh), else `<frame_index:04d>` under `track_mesh/`, `posed_mesh/` or `tpose_mesh/`.  The switches are read from the active
cfg and default to False.  The .ply is binary little-endian: float32 x y z per vertex, then per face one uchar 3 and three int32.
The reference's call of Blender afterwards (blend-weight replacement) is left out.  Without subdivision plain numpy: runs anywhere.
"""
import os

import numpy as np
import torch

from .. import config


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply(path, verts, faces):
    verts, faces = np.ascontiguousarray(_np(verts), '<f4').reshape(-1, 3), np.ascontiguousarray(_np(faces), '<i4').reshape(-1, 3)
    rec = np.empty(len(faces), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    rec['n'], rec['v'] = 3, faces
    header = ('ply\nformat binary_little_endian 1.0\n'
              f'element vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n'
              f'element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n')
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(verts.tobytes())
        fh.write(rec.tobytes())


def export_dotdict(output, filename):
    arrays = {k: _np(v) for k, v in output.items() if isinstance(v, (torch.Tensor, np.ndarray))}
    np.savez_compressed(filename, **arrays)


def export_mesh(verts, faces, filename='default.ply', subdivision=0, engine=None):
    if subdivision > 0:         # data_utils.py:252-254: Loop subdivision on the device (mesh_utils.loop_subdivision; needs the engine)
        from ..mesh_utils import loop_subdivision
        verts, faces = loop_subdivision(torch.as_tensor(_np(verts)) if not isinstance(verts, torch.Tensor) else verts,
                                        torch.as_tensor(_np(faces)) if not isinstance(faces, torch.Tensor) else faces, subdivision, engine=engine)
    if filename.endswith('.npz'):
        export_dotdict(dict(verts=verts, faces=faces), filename)
    elif filename.endswith('.ply'):
        write_ply(filename, verts, faces)
    else:
        raise NotImplementedError(f'Unrecognized output format for: {filename}')


class Visualizer:
    def __init__(self, result_dir=None):
        cfg = config.active_cfg()
        self.result_dir = result_dir or 'data/animation/{}/{}'.format(cfg.get('task', 'task'), cfg.get('exp_name', 'exp'))

    def result_paths(self, batch):
        """(npz path, ply path) of a batch's mesh"""
        cfg = config.active_cfg()
        can, tpose, posed, track = (bool(cfg.get(k, False)) for k in ('vis_can_mesh', 'vis_tpose_mesh', 'vis_posed_mesh', 'track_tpose_mesh'))
        item = lambda v: int(v.item()) if hasattr(v, 'item') else int(v)
        result_dir = self.result_dir
        if (item(batch['meta']['latent_index']) == -1 and tpose and track) or can:
            name = 'can_mesh'
        elif posed or tpose:
            result_dir = os.path.join(result_dir, 'track_mesh' if track else 'posed_mesh' if posed else 'tpose_mesh')
            name = '{:04d}'.format(item(batch['meta']['frame_index']))
        else:
            raise ValueError('mesh_visualizer: none of cfg.vis_can_mesh, vis_tpose_mesh, vis_posed_mesh is set')
        return os.path.join(result_dir, name + '.npz'), os.path.join(result_dir, name + '.ply')

    def visualize(self, output, batch):
        meta_path, mesh_path = self.result_paths(batch)
        os.makedirs(os.path.dirname(meta_path), exist_ok=True)
        export_dotdict(output, meta_path)
        export_mesh(output['verts'], output['faces'], filename=mesh_path)
        return meta_path, mesh_path

    def prepare_result_paths(self): pass

    def update_result_dir(self): pass

    def summarize(self): pass
