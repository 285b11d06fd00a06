"""Generate tests/golden/loss_wgrad_golden.npz (authoring container only: needs the reference checkout).

    python tests/golden/make_loss_wgrad_golden.py

Recorded: torch autograd through the REAL reference (oracle/ref_loader.py), fp32 on the CPU, SynergyNet() in eval() with
synth.make_synergy_state(loss_cases.SEED_SYN) on the five graph faces of loss_grad_cases.graph_inputs(), composed as
model_building.py:141-157 composes it:
  * w|<loss>|<state_dict key>: the gradient of the loss's .mean() -- 'total' is the sum of the five means -- with respect to every
    learnable tensor of forwardDirection.* / reverseDirection.* for total, loss_LMK_pointNet, loss_Param_S2 and loss_Param_S1S2.  Tensors
    of up to 4096 elements whole, every 499th element of the larger ones (loss_wgrad_cases.recorded_part; every 61st would need 0.9 MB).
  * loss_LMK_f0 and loss_Param_In: asserted here to reach no weight at all (autograd returns None for every tensor).
  * tie|<key>: loss_grad_cases.tie_case (max-pool ties in MLP_for) through the reference with that case's landmark basis, total, for
    forwardDirection.conv5.weight (every 61st element) and conv1.weight.
  * wgrad_faces: the batch_faces of loss_grad_golden.npz that loss_wgrad_cases.select_wgrad_faces keeps.
Every recorded tensor is computed a second time in float64 and must agree to 1e-5 x max |g| of the tensor.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import loss_cases as lc                   # noqa: E402
import loss_grad_cases as lg              # noqa: E402
import loss_wgrad_cases as lw             # noqa: E402
from oracle import ref_loader             # noqa: E402
from synergynet_amd import synth          # noqa: E402

worst = [0.0, '']


def agree(name, g32, g64):
    assert lg.same_classes(g32, g64), name
    r = lg.rel_to_max(g32, g64)
    if r > worst[0]:
        worst[:] = [r, name]
    assert r <= lg.CPU_BAR, (name, r)
    return np.asarray(g32, dtype=np.float32)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    g = dict(np.load(os.path.join(HERE, 'reference_outputs.npz'), allow_pickle=False))
    ggold = dict(np.load(lg.GOLDEN, allow_pickle=False))
    pack = synth.make_3dmm(int(g['seeds'][1]))
    ref = ref_loader.load_reference(pack)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    out = dict(torch_version=np.array(torch.__version__), graph_seed=np.array(lc.SEED_SYN), sample=np.array(lw.SAMPLE))
    keys = lw.learnable_keys()

    def load(model, sd, dt):
        model.float()
        for mod, prefix in zip((model.forwardDirection, model.reverseDirection), synth.SYNERGY_PREFIXES):
            own = mod.state_dict()
            mod.load_state_dict({k: t(np.asarray(sd[prefix + k])) if prefix + k in sd else v for k, v in own.items()})
        model.eval()
        if dt == torch.float64:
            model.double()

    def tensors(model):
        named = {}
        for mod, prefix in zip((model.forwardDirection, model.reverseDirection), synth.SYNERGY_PREFIXES):
            named.update({prefix + k: v for k, v in mod.named_parameters()})
        assert set(named) == set(keys), set(named) ^ set(keys)
        return [named[k] for k in keys]

    def graph_wgrads(model, inputs, dt, names):
        param, pool, target = inputs
        a, avgpool, gt = t(param, dt), t(pool, dt), t(target, dt)
        loss = {}
        vertex_lmk = model.reconstruct_vertex_62(a, dense=False)
        vertex_GT_lmk = model.reconstruct_vertex_62(gt, dense=False)
        loss['loss_LMK_f0'] = 0.05 * model.LMKLoss_3D(vertex_lmk, vertex_GT_lmk, kp=True)
        loss['loss_Param_In'] = 0.02 * model.ParamLoss(a, gt)
        vertex_lmk = vertex_lmk + 0.05 * model.forwardDirection(vertex_lmk, avgpool, a[:, 12:52], a[:, 52:62])
        loss['loss_LMK_pointNet'] = 0.05 * model.LMKLoss_3D(vertex_lmk, vertex_GT_lmk, kp=True)
        s2 = model.reverseDirection(vertex_lmk)
        loss['loss_Param_S2'] = 0.02 * model.ParamLoss(s2, gt, mode='only_3dmm')
        loss['loss_Param_S1S2'] = 0.001 * model.ParamLoss(s2, a, mode='only_3dmm')
        means = {k: loss[k].mean() for k in lc.LOSS_NAMES}
        means['total'] = sum(means.values())
        for z in lw.ZERO_LOSSES:
            assert not means[z].requires_grad, z                      # reaches no weight
        ps = tensors(model)
        res = {}
        for n in names:
            gr = torch.autograd.grad(means[n], ps, retain_graph=True, allow_unused=True)
            res[n] = {k: (np.zeros(tuple(p.shape)) if x is None else x.numpy()) for k, p, x in zip(keys, ps, gr)}
        return res

    sd = synth.make_synergy_state(lc.SEED_SYN)
    model = ref.SynergyNet()
    inputs = lg.graph_inputs()
    load(model, sd, torch.float32)
    g32 = graph_wgrads(model, inputs, torch.float32, lw.RECORDED)
    load(model, sd, torch.float64)
    g64 = graph_wgrads(model, inputs, torch.float64, lw.RECORDED)
    for n in lw.RECORDED:
        for k in keys:
            out[lw.fixture_key(n, k)] = lw.recorded_part(agree(f'{n} {k}', g32[n][k], g64[n][k]))
        big = max(keys, key=lambda k: np.abs(g32[n][k]).max())
        print(n, 'largest max |g| %.3g (%s); exactly zero tensors:' % (np.abs(g32[n][big]).max(), big), [k for k in keys if not g32[n][k].any()])
    print('worst fp32 / fp64 disagreement on the graph faces: %.3g (%s), bar %g' % (worst[0], worst[1], lg.CPU_BAR))

    # the tie case: the same reference with that case's landmark basis and whitening mean
    tpack, tsd, *tin = lg.tie_case(pack, sd, ggold['batch_faces'])
    kp = np.asarray(tpack['keypoints'])
    u = np.asarray(tpack['u_shp'], dtype=np.float64) + np.asarray(tpack['u_exp'], dtype=np.float64)
    tie = {}
    for dt in (torch.float32, torch.float64):
        load(model, tsd, dt)
        for name, val in (('u_base', u[kp]), ('w_shp_base', np.asarray(tpack['w_shp'])[kp]), ('w_exp_base', np.asarray(tpack['w_exp'])[kp]),
                          ('param_mean', np.asarray(tpack['param_mean']))):
            getattr(model, name).data = t(val, dt).reshape(getattr(model, name).shape)
        tie[dt] = graph_wgrads(model, tin, dt, ('total',))['total']
    for k in lw.TIE_KEYS:
        out[f'tie|{k}'] = lw.recorded_part(agree(f'tie {k}', tie[torch.float32][k], tie[torch.float64][k]), lw.TIE_SAMPLE)

    out['wgrad_faces'], rejected = lw.select_wgrad_faces(pack, sd, ggold['batch_faces'])
    print('wgrad faces', out['wgrad_faces'].tolist(), 'rejected', rejected)
    B = len(out['wgrad_faces'])
    batch = lw.wgrad_inputs(out['wgrad_faces'], B)
    up = lw.total_upstream(B)
    e = lw.worst_rel(lw.WHead(pack, sd, torch.float32).wvjp(*batch, *up), lw.WHead(pack, sd).wvjp(*batch, *up))
    print('the batch of the %d selected faces: fp32 against float64 %.3g (%s)' % (B, e[0], e[1]))
    assert e[0] <= lg.CPU_BAR

    np.savez_compressed(lw.GOLDEN, **out)
    print('wrote', lw.GOLDEN, os.path.getsize(lw.GOLDEN), 'bytes')
    assert os.path.getsize(lw.GOLDEN) < 512 << 10


if __name__ == '__main__':
    main()
