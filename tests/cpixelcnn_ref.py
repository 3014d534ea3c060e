"""Torch restatement of the CPixelCNN baseline's training-mode forward (reference: models/cpixelcnn.py) over a state dict.
float64 by default; the short-batch reference test also runs it in float32 to measure the reference's own rounding.
Shared by test_cpixelcnn_gpu.py and the short-batch tests."""
import torch
import torch.nn.functional as F


def ref_module(sd, classes, dtype=torch.float64):
    """ConditionalGatedPixelCNN's train-mode forward (cpixelcnn.py) over a state dict -> a module whose call gives the loss;
    parameters in `dtype` (float64 unless told otherwise)."""
    import torch.nn as nn
    p = {k: nn.Parameter(v.to(dtype).clone()) for k, v in sd.items() if v.is_floating_point() and 'running' not in k}
    with torch.no_grad():                     # mask 'A' zeroes the parameters in place (cpixelcnn.py:42-44): the masked
        p['layers.0.vert_stack.weight'][:, :, -1] = 0        # taps still receive a gradient, as in the reference
        p['layers.0.horiz_stack.weight'][:, :, :, -1] = 0
    layers = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('layers.'))

    class R(nn.Module):
        def __init__(self):
            super().__init__()
            for k, v in p.items():
                self.register_parameter(k.replace('.', '__'), v)

        def named_parameters(self, *a, **k):
            return [(n.replace('__', '.'), v) for n, v in super().named_parameters()]

        def forward(self, codes, lab):
            P = {n.replace('__', '.'): v for n, v in super().named_parameters()}

            def bn(x, pre):
                return F.batch_norm(x, None, None, P[pre + '.weight'], P[pre + '.bias'], True, 0.1, 1e-5)

            def gate(x, pre):
                a, b = x.chunk(2, 1)
                return torch.relu(bn(a, pre + '.bn')) * torch.sigmoid(b)
            x = P['embedding.weight'][codes].permute(0, 3, 1, 2)
            xv = xh = x
            for i in range(layers):
                q = f'layers.{i}'
                k = 7 if i == 0 else 3
                wv, wh = P[q + '.vert_stack.weight'], P[q + '.horiz_stack.weight']
                e = P[q + '.class_cond_embedding.weight'][lab][:, :, None, None]
                hv = F.conv2d(xv, wv, P[q + '.vert_stack.bias'], padding=(k // 2, k // 2))[:, :, :xv.size(-1), :]
                ov = gate(hv + e, q + '.gate_v')
                hh = F.conv2d(xh, wh, P[q + '.horiz_stack.bias'], padding=(0, k // 2))[:, :, :, :xh.size(-2)]
                v2h = F.conv2d(hv, P[q + '.vert_to_horiz.weight'], P[q + '.vert_to_horiz.bias'])
                oh = gate(v2h + hh + e, q + '.gate_h')
                r = bn(F.conv2d(oh, P[q + '.horiz_resid.0.weight'], P[q + '.horiz_resid.0.bias']), q + '.horiz_resid.1')
                xh = r + xh if i > 0 else r
                xv = ov
            h0 = torch.relu(bn(F.conv2d(xh, P['output_conv.0.weight'], P['output_conv.0.bias']), 'output_conv.1'))
            logits = F.conv2d(h0, P['output_conv.3.weight'], P['output_conv.3.bias'])
            return F.cross_entropy(logits, codes)
    return R()
