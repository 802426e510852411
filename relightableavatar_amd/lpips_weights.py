"""The LPIPS (AlexNet) weight set: shapes, constants, and the one table that maps a user's state-dict keys onto them.

The pretrained weights are not shipped and not fetched: a user exports `lpips.LPIPS().state_dict()` where the package is installed
 and hands it to Engine.lpips_load.  Three key layouts are accepted, in this order per tensor:

    neutral        conv{k}.weight / conv{k}.bias, lin{k}.weight, shift, scale                         k = 0..4
    lpips          net.slice{k+1}.{i}.weight / .bias, lin{k}.model.1.weight, scaling_layer.shift / .scale
    torchvision    features.{i}.weight / .bias (alexnet().state_dict()), together with lin* keys of either spelling

with i = 0, 3, 6, 8, 10 the index of the convolution in torchvision's `features`.  The lpips and torchvision spellings are written from
memory of the published sources: neither package is installed where this project is built, so they are NOT verified against them.
"""
import numpy as np
import torch

TAPS = 5
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
_FEATURE_INDEX = (0, 3, 6, 8, 10)


def key_table():
    """{slot: (accepted key names, shape, required)}; a tensor is accepted in any shape with the right element count"""
    t = {}
    for k, shp in enumerate(CONV_SHAPES):
        i = _FEATURE_INDEX[k]
        t[f'conv{k}.weight'] = ((f'conv{k}.weight', f'net.slice{k + 1}.{i}.weight', f'features.{i}.weight'), shp, True)
        t[f'conv{k}.bias'] = ((f'conv{k}.bias', f'net.slice{k + 1}.{i}.bias', f'features.{i}.bias'), (shp[0],), True)
        t[f'lin{k}.weight'] = ((f'lin{k}.weight', f'lin{k}.model.1.weight', f'lins.{k}.model.1.weight'), (1, shp[0], 1, 1), True)
    t['shift'] = (('shift', 'scaling_layer.shift'), (1, 3, 1, 1), False)
    t['scale'] = (('scale', 'scaling_layer.scale'), (1, 3, 1, 1), False)
    return t


def _expected():
    return '; '.join(f'{" | ".join(names)} {shape}' + ('' if req else ' (optional)') for names, shape, req in key_table().values())


def resolve(state_dict):
    """-> {slot: contiguous float32 numpy array} for every slot of key_table() (shift / scale default to the lpips constants).
    A missing key or a wrong element count raises KeyError / ValueError that lists the expected names and shapes."""
    out, missing, wrong = {}, [], []
    for slot, (names, shape, required) in key_table().items():
        found = [n for n in names if n in state_dict]
        if not found:
            if required:
                missing.append(slot)
            else:
                out[slot] = np.asarray(SHIFT if slot == 'shift' else SCALE, np.float32)
            continue
        v = state_dict[found[0]]
        v = v.detach().to('cpu', torch.float32).numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)
        if v.size != int(np.prod(shape)) or (v.ndim == len(shape) and tuple(v.shape) != tuple(shape)):
            wrong.append(f'{found[0]} has shape {tuple(v.shape)}, expected {shape}')
            continue
        out[slot] = np.ascontiguousarray(v, np.float32).reshape(-1)
    if missing:
        raise KeyError(f'lpips weights: missing {", ".join(missing)}.  Expected keys (any one spelling each) and shapes: {_expected()}')
    if wrong:
        raise ValueError(f'lpips weights: {"; ".join(wrong)}.  Expected keys (any one spelling each) and shapes: {_expected()}')
    if np.any(out['scale'] == 0):
        raise ValueError('lpips weights: a zero scale')
    return out
