#!/usr/bin/env python3
"""Golden camera helpers of the rasteriser, made by running the REFERENCE's own get_ndc_perspective_matrix, make_rotation_y and
make_rotation (lib/utils/raster_utils.py) on the CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_raster.py            # writes raster.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_raster.py --check    # recomputes and compares with the committed file

The reference's module imports nvdiffrast and opens a GL context through log_utils.run at import time; neither exists here.  The shim
 gets a stub `nvdiffrast.torch` in sys.modules and log_utils.run is patched out before the import, so that only
the three pure functions run.  Nothing of nvdiffrast's is recorded: there is no output of it to be at parity with (DESIGN.md
section 25).  The reference never travels: only this fixture is committed.
"""
import argparse
import os
import sys
import types
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden import install_reference

OUT = 'raster.npz'


def inputs():
    rng = np.random.default_rng(2025)
    K2 = np.array([[612.5, 0, 255.25], [0, 608.75, 259.5], [0, 0, 1]], np.float32)
    K3 = np.stack([K2, K2 * np.float32(0.5), K2 + np.float32(3.0)]).astype(np.float32)
    ang = rng.uniform(-3.0, 3.0, (3, 5)).astype(np.float32)
    return dict(K2=K2, K3=K3, H=np.int64(480), W=np.int64(640), rx=ang[0], ry=ang[1], rz=ang[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    args = ap.parse_args()
    install_reference()
    stub = types.ModuleType('nvdiffrast')
    stub.torch = MagicMock(name='nvdiffrast.torch')
    sys.modules['nvdiffrast'], sys.modules['nvdiffrast.torch'] = stub, stub.torch
    from lib.utils import log_utils
    log_utils.run = lambda *a, **k: None
    from lib.utils import raster_utils as R
    arrs = inputs()
    H, W = int(arrs['H']), int(arrs['W'])
    t = lambda k: torch.from_numpy(arrs[k].copy())
    arrs['ndc_K2_torch'] = R.get_ndc_perspective_matrix(t('K2'), H, W).numpy()
    arrs['ndc_K3_torch'] = R.get_ndc_perspective_matrix(t('K3'), H, W).numpy()
    arrs['ndc_K2_numpy'] = R.get_ndc_perspective_matrix(arrs['K2'].copy(), H, W)
    arrs['ndc_K3_numpy'] = R.get_ndc_perspective_matrix(arrs['K3'].copy(), H, W)
    arrs['rot_y'] = R.make_rotation_y(t('ry')).numpy()
    arrs['rot_xyz'] = R.make_rotation(t('rx'), t('ry'), t('rz')).numpy()
    arrs['rot_x'] = R.make_rotation(rx=t('rx')).numpy()
    arrs['rot_z'] = R.make_rotation(rz=t('rz')).numpy()
    assert all(np.isfinite(a).all() for a in arrs.values())
    path = os.path.join(HERE, OUT)
    if args.check:
        old = np.load(path)
        assert sorted(old.files) == sorted(arrs), 'key sets differ'
        for k, a in arrs.items():
            assert np.array_equal(old[k], a), k
        print(f'{OUT}: {len(arrs)} arrays equal')
        return
    np.savez_compressed(path, **arrs)
    print(f'wrote {path}: {len(arrs)} arrays, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
