"""arch_search/eff_pred.py: the cost of a candidate, as multiply-accumulates of one forward."""
from ..models.pose_supermobilenet import SuperLitePose


def _conv_out(size, k, stride):
    return (size + 2 * (k // 2) - k) // stride + 1


class EfficiencyEvaluator(object):
    """``predict_eff(cfg_arch)``: the multiply-accumulates, in units of 1e9, of one forward of the sub-network on one
    ``img_size`` x ``img_size`` image.  Every convolution and transposed convolution counts ``out_pixels * Cout *
    Cin/groups * k * k`` (a transposed convolution by its OUTPUT pixels too); BatchNorm, activations and bias count
    nothing.  Computed in Python from the channel bookkeeping of ``SuperLitePose._sub_plan``: nothing is built or run.

    The reference's number comes from ``ptflops`` on an instantiated model.  ``ptflops`` is not available here, counts
    more than multiply-accumulates (BatchNorm and activations, and transposed convolutions by their input pixels) and
    hands the value over parsed from a rounded string ('1.23 GMac').  This value is therefore NOT pinned against it: a
    constraint tuned on the reference's scale (``set_efficiency_constraint(8)`` in search.py) needs re-tuning."""

    def __init__(self, cfg):
        self.cfg = cfg
        self._super = SuperLitePose(cfg)            # host bookkeeping only: no tensors, no device

    def layers(self, cfg_arch):
        """(name, out_h, out_w, Cout, Cin per group, k) of every convolution of the sub-network, in forward order."""
        plan = self._super._sub_plan(cfg_arch)
        reso = int(cfg_arch['img_size'])
        L = []
        h = _conv_out(reso, 3, 2)
        L.append(('first.0.0', h, h, 32, 3, 3))
        L.append(('first.1.0', h, h, 32, 1, 3))
        L.append(('first.2', h, h, plan['c0'], 32, 1))
        sizes = [h]
        for s, blocks in enumerate(plan['stages']):
            for b, blk in enumerate(blocks):
                p = 'stage.%d.%d' % (s, b)
                stride = self._super.stages[s][b]['stride']
                L.append((p + '.inv.0', h, h, blk['mid'], blk['inp'], 1))
                h = _conv_out(h, blk['k'], stride)
                L.append((p + '.depth_conv.0', h, h, blk['mid'], 1, blk['k']))
                L.append((p + '.point_conv.0', h, h, blk['oup'], blk['mid'], 1))
            sizes.append(h)
        ch, fl = plan['channel'], plan['filters']
        h = sizes[-1]
        for i in range(3):
            h = 2 * h                                # ConvTranspose2d(kernel 4, stride 2, padding 1)
            L.append(('deconv_refined.%d' % i, h, h, fl[i], ch[-1] if i == 0 else fl[i - 1], 4))
            L.append(('deconv_raw.%d' % i, h, h, fl[i], ch[-i - 2], 4))
            if i > 0:
                for name, cin in (('final_refined', fl[i]), ('final_raw', ch[-i - 3])):
                    p = '%s.%d.conv' % (name, i - 1)
                    L.append((p + '.0', h, h, cin, 1, 5))
                    L.append((p + '.3', h, h, self._super.final_channel[i - 1], cin, 1))
        return L

    def macs(self, cfg_arch):
        return sum(oh * ow * cout * cin * k * k for _, oh, ow, cout, cin, k in self.layers(cfg_arch))

    def predict_eff(self, cfg_arch):
        return self.macs(cfg_arch) / 1e9
