"""Plain fp64 restatement of the gradient of the training loss with respect to the stage output, for the tests of
lp_pose_loss_grad (tests/test_gpu_loss_grad.py, tests/test_loss_grad_cpu.py) and for the fixture
tests/golden/golden_loss_grad.npz, which stores its values beside autograd's through the real lib/core/loss.py.  numpy only.

As in tests/_loss_ref.py the functions take the fp32 inputs widened to fp64 and round nothing: a device result is held to
ONE fp32 rounding of these values.  Sums run in a stated order: a person's joints in slot order, the columns of a push row in
person order, and the slots that share a cell in (person, joint) order."""
import numpy as np


def heat_grad(pred, gt, mask, factor, g):
    """d(g * heat_loss) / d pred for one image: pred, gt [J,R,R], mask [R,R] (fp32), ``factor`` and the upstream ``g`` fp32
    widened -> fp64 [J,R,R]: k * ((pred - gt) * mask) with k = g * factor * 2 / (J R R)."""
    d = pred.astype(np.float64) - gt.astype(np.float64)
    k = ((float(np.float32(g)) * float(np.float32(factor))) * 2.0) / d.size
    return k * (d * mask.astype(np.float64)[None])


def push_slope(d, loss_type):
    """f'(d) of the push term: f = exp(-d^2) or max(1 - |d|, 0)."""
    if loss_type == 'exp':
        return (-2.0 * d) * float(np.exp(-(d * d)))
    if abs(d) < 1.0:
        return -1.0 if d > 0.0 else (1.0 if d < 0.0 else 0.0)
    return 0.0


def tag_grad(tagmaps, joints, loss_type, push_factor, pull_factor, g_push, g_pull):
    """d(g_push * push + g_pull * pull) / d tagmaps for one image, push and pull as _loss_ref.tag_loss gives them: tagmaps
    fp32 [K,R,R], joints int [M,J,2], factors and upstream values fp32 widened, None for an upstream that is absent ->
    fp64 [K,R,R], zero wherever no counting slot points."""
    flat = tagmaps.astype(np.float64).reshape(-1)
    grad = np.zeros(flat.size, np.float64)
    slots, stats = [], {}
    for p, person in enumerate(joints):
        own = [int(i) for i, v in person if v > 0 and 0 <= int(i) < flat.size]
        if not own:
            continue
        s = 0.0
        for i in own:
            s += flat[i]
        stats[p] = (len(own), s / len(own))
        slots += [(p, i) for i in own]
    persons = len(stats)
    pc = float(max(persons, 1))
    den = max((pc - 1.0) * pc, 1.0)
    push_on = g_push is not None and persons >= 2
    wpull = None if g_pull is None else (float(np.float32(g_pull)) * float(np.float32(pull_factor))) * 2.0
    wpush = float(np.float32(g_push)) * float(np.float32(push_factor)) if push_on else None
    dsum = {}
    if push_on:
        for p, (_, mp) in stats.items():
            acc = 0.0
            for q, (_, mq) in stats.items():
                acc += push_slope(mp - mq, loss_type)
            dsum[p] = acc
    seen = set()
    for p, i in slots:                                # (person, joint) order: a cell's first slot starts its sum
        cnt, mean = stats[p]
        v = 0.0
        if wpull is not None:
            v = (wpull * (flat[i] - mean)) / (cnt * pc)
        if push_on:
            v += (wpush * dsum[p]) / (den * cnt)
        grad[i] = grad[i] + v if i in seen else v
        seen.add(i)
    return grad.reshape(tagmaps.shape)


def push_gaps(tagmaps, joints):
    """|mu_p - mu_q| of every pair of distinct counting persons of one image (the arguments of the push slope)."""
    flat = tagmaps.astype(np.float64).reshape(-1)
    means = []
    for person in joints:
        own = [flat[int(i)] for i, v in person if v > 0 and 0 <= int(i) < flat.size]
        if own:
            s = 0.0
            for t in own:
                s += t
            means.append(s / len(own))
    return [abs(a - b) for x, a in enumerate(means) for y, b in enumerate(means) if x != y]
