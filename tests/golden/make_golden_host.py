"""Generates tests/golden/host_golden.npz: what the reference's own PYTHON classes compute on the inputs of
tests/test_oracle_vs_reference.py's host-mirror tests, so that those tests run without the reference's sources.

  ann<i>_*   openpifpaf.Annotation (COCO person): data / joint_scales in, score, bbox, json_data (JSON text) and
             inverse_transform(meta) -> data, joint_scales out, for five random poses (default_rng(11))
  head_*     openpifpaf.network.heads.CompositeField4 for the CIF and CAF metas: the input features, the 1x1
             convolution's weight / bias (torch.manual_seed(0), this package's initialisation) and the head's output

    python tests/golden/make_golden_host.py          (build container only: needs the reference's sources)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import reference_python                       # noqa: E402

OUT = os.path.join(HERE, 'host_golden.npz')
ANNOTATION_META = {'offset': np.array((-7.0, 12.0)), 'scale': np.array((0.8, 0.75)), 'hflip': True,
                   'rotation': {'angle': 0.0, 'width': None, 'height': None}, 'width_height': np.array((500, 375)),
                   'valid_area': np.array((0.0, 0.0, 499.0, 374.0))}


def annotation_inputs():
    rng = np.random.default_rng(11)
    out = []
    for _ in range(5):
        data = rng.uniform(0, 200, (17, 3)).astype(np.float32)
        data[:, 2] = rng.uniform(0, 1, 17) * (rng.random(17) > 0.3)
        scales = rng.uniform(1, 9, 17).astype(np.float32)
        out.append((data, scales))
    return out


def head_inputs():
    """-> (features [2,64,7,9], {name: this package's CompositeField4}) with the weights of torch.manual_seed(0)."""
    import torch
    from openpifpaf_amd import headmeta, network
    torch.manual_seed(0)
    metas = headmeta.cocokp_metas()
    x = torch.randn(2, 64, 7, 9)
    return x, metas, {name: network.CompositeField4(m, 64).eval() for name, m in zip(('cif', 'caf'), metas)}


def main():
    import torch
    opp = reference_python.load()
    from openpifpaf_amd import constants
    out = {}
    for i, (data, scales) in enumerate(annotation_inputs()):
        a = opp.Annotation(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON,
                           score_weights=constants.COCO_PERSON_SCORE_WEIGHTS)
        a.data[:] = data
        a.joint_scales[:] = scales
        inv = a.inverse_transform(ANNOTATION_META)
        out.update({'ann%d_data' % i: data, 'ann%d_scales' % i: scales, 'ann%d_score' % i: np.float64(a.score),
                    'ann%d_bbox' % i: np.asarray(a.bbox(), dtype=np.float64),
                    'ann%d_json' % i: np.array(json.dumps(a.json_data())),
                    'ann%d_inv_data' % i: np.asarray(inv.data), 'ann%d_inv_scales' % i: np.asarray(inv.joint_scales)})
    x, metas, mine = head_inputs()
    out['head_x'] = x.numpy()
    ref_cif = opp.headmeta.Cif('cif', 'cocokp', keypoints=metas[0].keypoints, sigmas=metas[0].sigmas,
                               pose=np.asarray(metas[0].pose), draw_skeleton=metas[1].skeleton)
    ref_caf = opp.headmeta.Caf('caf', 'cocokp', keypoints=metas[0].keypoints, sigmas=metas[0].sigmas,
                               pose=np.asarray(metas[0].pose), skeleton=metas[1].skeleton)
    for name, ref_meta in (('cif', ref_cif), ('caf', ref_caf)):
        ref_meta.base_stride, ref_meta.upsample_stride = 16, 2
        ref = opp.network.heads.CompositeField4(ref_meta, 64).eval()
        ref.conv.load_state_dict(mine[name].conv.state_dict())
        with torch.no_grad():
            y = ref(x)
        out['head_%s_weight' % name] = mine[name].conv.weight.detach().numpy()
        out['head_%s_bias' % name] = mine[name].conv.bias.detach().numpy()
        out['head_%s_out' % name] = y.numpy()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
