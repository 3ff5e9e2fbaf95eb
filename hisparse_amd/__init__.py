"""hisparse_amd — MI355X-native SpMV engine behind HiSparse's host interface.

Layout:
  host.py      ctypes face of libhisparse_host.so  (CSR ingest, CSR -> CPSR formatter, channel assembly)
  device.py    ctypes face of libhisparse_hip.so   (the drop-in C-ABI: load / run / read back, gfx950 kernels)
  rows.py      ctypes face of include/hisparse_rows.h (the row softmax over a CSR pattern, forward and backward)
  wide.py      ctypes face of include/hisparse_wide.h (SDDMM, SpMM and transposed SpMM over a CSR pattern, row-major features)
  attention.py ctypes face of include/hisparse_attention.h (scores, row softmax and weighted sum over a CSR pattern in one call)
  attention_backward.py ctypes face of include/hisparse_attention_backward.h (the backward of that step, from lse to gQ, gK and gV)
  heads.py     ctypes face of include/hisparse_heads.h (multi-head attention over a CSR pattern, forward and backward, all heads per call)
  heads16.py   ctypes face of include/hisparse_heads_bf16.h (the same object with bf16 operands)
  heads_bias.py ctypes face of include/hisparse_heads_bias.h (the same object with a per-entry, per-head additive bias and its gradient)
  heads_dropout.py ctypes face of include/hisparse_heads_dropout.h (the same object with dropout on the attention weights, no mask stored)
  heads16_dropout.py ctypes face of include/hisparse_heads_dropout_bf16.h (that bias and dropout over bf16 operands)
  gat.py       ctypes face of include/hisparse_gat.h (the same object with GAT's additive scores, el[row] + er[col] through a LeakyReLU)
  gatv2.py     ctypes face of include/hisparse_gatv2.h (the same object with GATv2's score, a . LeakyReLU(XD[row] + XS[col]), and the gradient of a)
  aggregate.py ctypes face of include/hisparse_aggregate.h (sum, mean, max and min of the neighbours' rows on wide.py's object, with the arg-based backward)
  datasets.py  the reference's benchmark matrices as seeded stand-ins
  sharding.py  row-block sharding of one matrix across the GPUs of a node (+ RCCL gather of y)
  csrc/        C++ / HIP sources of the two libraries and the `benchmark` driver
"""
from . import host  # noqa: F401
from . import device  # noqa: F401
from . import datasets  # noqa: F401
from . import rows  # noqa: F401
from . import wide  # noqa: F401
from . import attention  # noqa: F401
from . import attention_backward  # noqa: F401
from . import heads  # noqa: F401
from . import heads16  # noqa: F401
from . import heads_bias  # noqa: F401
from . import heads_dropout  # noqa: F401
from . import heads16_dropout  # noqa: F401
from . import gat  # noqa: F401
from . import gatv2  # noqa: F401
from . import aggregate  # noqa: F401

__all__ = ["host", "device", "datasets", "rows", "wide", "attention", "attention_backward", "heads", "heads16", "heads_bias", "heads_dropout", "heads16_dropout", "gat", "gatv2", "aggregate"]
