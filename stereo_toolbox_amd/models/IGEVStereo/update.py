"""The recurrent cell of the iterative families on csrc/convgru.hip.

`ConvGRU` is a drop-in for the class the reference defines, word for word the same, in IGEVStereo/update.py:25-40,
RAFTStereo/update.py:16-32, DEFOMStereo/update.py:18-37, StereoAnywhere/update.py:46-62 and FoundationStereo/update.py:33-47:
same constructor, forward signature and state-dict keys (`convz / convr / convq . weight / bias`), so their checkpoints load.
One class object serves all five packages.  The rest of the update blocks (motion encoders, heads, pool2x / interp,
BasicMultiUpdateBlock, SepConvGRU) is not built; RaftConvGRU / SelectiveConvGRU live in models/SelectiveStereo.
"""
import torch.nn as nn

from ... import ops


class ConvGRU(nn.Module):
    def __init__(self, hidden_dim, input_dim, kernel_size=3):
        super().__init__()
        if kernel_size != 3:
            raise ops.StxError(f"ConvGRU: kernel_size {kernel_size}; the gfx950 cell serves 3x3 only")
        # nn.Conv2d holds the parameters (keys, shapes and default initialisation of the reference); it is never called
        self.convz = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convr = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convq = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)

    def forward(self, h, cz, cr, cq, *x_list):
        return ops.convgru(h, cz, cr, cq, x_list, self.convz.weight, self.convz.bias, self.convr.weight, self.convr.bias,
                           self.convq.weight, self.convq.bias)
