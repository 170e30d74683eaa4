"""The reference's graph transformer (src/transformer/{model,gt_conv,mlp}.py) as parameter containers whose forward runs on
the HIP kernels of csrc/gt_policy.hip, plus the positional-encoding helper of MLAgents.compute_encodings."""
from .model import GTConv, GraphTransformerNet, MLP  # noqa: F401
from .encoding import laplacian_pe, cached_laplacian_pe  # noqa: F401
