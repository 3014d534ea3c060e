#!/usr/bin/env python3
"""Driver counterpart of the reference's src/test_pixelcnn.py:42-84: the trained MCPixelCNN / CPixelCNN over the code maps of
the frozen VQ-VAE (<ae_tag>_best.pt; `ae.encode(img)[2]` replaces the image, :74-75), metrics Loss + NLL (:26), the trailing
n = 1 append (:80), the 'test' line and output/result/<model_tag>.pt.  No grids.  Shared parts: compat/_evaluate.py."""
from _evaluate import EvalDriver


class PixelCNNTest(EvalDriver):
    metric_names = ['Loss', 'NLL']
    runs_prefix = 'train'                                 # test_pixelcnn.py:55

    def prepare(self, input, ae):                         # test_pixelcnn.py:74-75
        _, _, code = ae.encode(input['img'])
        return dict(input, img=code.detach())


if __name__ == '__main__':
    PixelCNNTest().main(('mcpixelcnn', 'cpixelcnn'))
