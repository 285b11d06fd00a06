"""Generate tests/golden/loss_golden.npz (authoring container only: needs the reference checkout).

    python tests/golden/make_loss_golden.py

Everything recorded here is computed by the REAL reference, imported from where it lies (oracle/ref_loader.py), in torch fp32 on the CPU:
  * loss_definition.WingLoss() / ParamLoss() on the deterministic inputs of tests/loss_cases.py (rebuilt there from integers, so only
    their checksums and the reference's results are stored):  wing_B{B}_n{n}_{variant}, param_B{B}_{mode}[_same]
  * the reference's SynergyNet() with synth.make_synergy_state(seed) loaded into forwardDirection / reverseDirection, its
    reconstruct_vertex_62, LMKLoss_3D and ParamLoss composed exactly as model_building.py:141-157 composes them, on 5 faces: inputs
    graph_param / graph_target / graph_pool, intermediates graph_lmk / graph_lmk_gt / graph_lmk_refined / graph_param_rev, and the five
    weighted losses graph_loss_*.  Predictions and targets are drawn independently, so the landmarks differ by several pixels.
  * utils.ddfa.CenterCrop(m, mode='test') on loss_cases.ramp() at m = 5, 0, 59, 60:  crop_m{m}
Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import loss_cases as lc                   # noqa: E402
from oracle import ref_loader             # noqa: E402
from synergynet_amd import synth          # noqa: E402


def ref_module(name):
    """A further module of the reference, imported from where it lies.  load_reference takes the reference's modules out of sys.modules
    again and keeps them in ref_loader._REF_MODULES: they (its `utils` package, the cv2 stub) are put back for the import only."""
    import importlib
    keep = dict(sys.modules)
    sys.modules.update(ref_loader._REF_MODULES)
    sys.modules.setdefault('cv2', type(sys)('cv2'))
    sys.path.insert(0, ref_loader.REF_ROOT)
    try:
        return importlib.import_module(name)
    finally:
        sys.path.remove(ref_loader.REF_ROOT)
        for k in list(sys.modules):
            if k not in keep:
                del sys.modules[k]
        sys.modules.update(keep)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    g = dict(np.load(os.path.join(HERE, 'reference_outputs.npz'), allow_pickle=False))
    pack = synth.make_3dmm(int(g['seeds'][1]))
    ref = ref_loader.load_reference(pack)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = dict(torch_version=np.array(torch.__version__))

    wing_ref, param_ref = ref.WingLoss(), ref.ParamLoss()
    for name in lc.wing_case_names():
        B, n, v = lc.parse_wing_case(name)
        pred, target = lc.wing_inputs(B, n, v)
        with torch.no_grad():
            r = wing_ref(t(pred), t(target), kp=True)
        out[name] = np.float32(r.item())
        out[name + '_sum'] = lc.checksum(pred, target)
        d = np.abs(target.astype(np.float64) - pred.astype(np.float64))
        print(name, float(out[name]), 'restated', float(lc.wing(pred, target)), 'log / linear / neither:',
              int((d < 10).sum()), int((d >= 10).sum()), int(np.isnan(d).sum()))
    for B in lc.PARAM_B:
        for mode in ('normal', 'only_3dmm'):
            for same in (False, True):
                a, b = lc.param_inputs(B, same)
                with torch.no_grad():
                    r = param_ref(t(a), t(b), mode=mode).numpy()
                key = f'param_B{B}_{mode}' + ('_same' if same else '')
                out[key], out[key + '_sum'] = r.astype(np.float32), lc.checksum(a, b)
                print(key, r[:3], 'restated', lc.param_loss(a, b, mode)[:3])

    # graph level
    model = ref.SynergyNet()              # random backbone (unused here); the MLPs get the synthetic state
    sd = synth.make_synergy_state(lc.SEED_SYN)
    for mod, prefix in zip((model.forwardDirection, model.reverseDirection), synth.SYNERGY_PREFIXES):
        own = mod.state_dict()
        mod.load_state_dict({k: t(np.asarray(sd[prefix + k])) if prefix + k in sd else v for k, v in own.items()})
    model.eval()
    param, target = synth.make_params(5, lc.SEED_GRAPH_PARAM), synth.make_params(5, lc.SEED_GRAPH_TARGET)
    pool = np.abs(np.random.default_rng(lc.SEED_GRAPH_POOL).standard_normal((5, 1280))).astype(np.float32)
    with torch.no_grad():
        a, gt, avgpool = t(param), t(target), t(pool)
        loss = {}
        vertex_lmk = model.reconstruct_vertex_62(a, dense=False)
        vertex_GT_lmk = model.reconstruct_vertex_62(gt, dense=False)
        loss['loss_LMK_f0'] = 0.05 * model.LMKLoss_3D(vertex_lmk, vertex_GT_lmk, kp=True)
        loss['loss_Param_In'] = 0.02 * model.ParamLoss(a, gt)
        point_residual = model.forwardDirection(vertex_lmk, avgpool, a[:, 12:52], a[:, 52:62])
        lmk0 = vertex_lmk.clone()
        vertex_lmk = vertex_lmk + 0.05 * point_residual
        loss['loss_LMK_pointNet'] = 0.05 * model.LMKLoss_3D(vertex_lmk, vertex_GT_lmk, kp=True)
        s2 = model.reverseDirection(vertex_lmk)
        loss['loss_Param_S2'] = 0.02 * model.ParamLoss(s2, gt, mode='only_3dmm')
        loss['loss_Param_S1S2'] = 0.001 * model.ParamLoss(s2, a, mode='only_3dmm')
    out.update(graph_param=param, graph_target=target, graph_pool=pool, graph_lmk=lmk0.numpy(), graph_lmk_gt=vertex_GT_lmk.numpy(),
               graph_lmk_refined=vertex_lmk.numpy(), graph_param_rev=s2.numpy(), graph_seed=np.array(lc.SEED_SYN))
    for k in lc.LOSS_NAMES:
        out['graph_' + k] = loss[k].numpy().astype(np.float32)
    d = np.abs(out['graph_lmk'] - out['graph_lmk_gt'])
    print('graph: |landmark difference| mean %.2f max %.2f px, share >= omega %.2f' % (d.mean(), d.max(), (d >= 10).mean()))
    assert d.mean() > 2.0 and 0.02 < (d >= 10).mean() < 0.98            # several pixels, both branches
    restated = lc.graph_losses(param, target, out['graph_lmk'], out['graph_lmk_gt'], out['graph_lmk_refined'], out['graph_param_rev'])
    for k, r in zip(lc.LOSS_NAMES, restated):
        print(k, out['graph_' + k], 'restated', r)

    # CenterCrop
    ddfa = ref_module('utils.ddfa')
    img = lc.ramp()[0]
    for m in lc.CROP_MARGINS:
        chw = ddfa.ToTensor()(img)
        got = ddfa.CenterCrop(m, mode='test')(chw)
        out[f'crop_m{m}'] = np.ascontiguousarray(got.numpy().transpose(1, 2, 0)).astype(np.uint8)
        print('crop margin', m, 'non-zero pixels', int(out[f'crop_m{m}'].any(2).sum()))
    out['crop_sum'] = lc.checksum(img)

    path = os.path.join(HERE, 'loss_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 400 << 10


if __name__ == '__main__':
    main()
