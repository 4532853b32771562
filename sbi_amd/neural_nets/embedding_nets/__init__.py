from sbi_amd.neural_nets.embedding_nets.fully_connected import FCEmbedding  # noqa: F401
from sbi_amd.neural_nets.embedding_nets.permutation_invariant import PermutationInvariantEmbedding  # noqa: F401
from sbi_amd.neural_nets.embedding_nets.cnn import (  # noqa: F401
    CNNEmbedding,
    calculate_filter_output_size,
    get_new_cnn_output_size,
)
from sbi_amd.neural_nets.embedding_nets.lru import LRU, LRUBlock, LRUEmbedding  # noqa: F401
from sbi_amd.neural_nets.embedding_nets.causal_cnn import (  # noqa: F401
    CausalCNNEmbedding,
    WaveNetSRLikeAggregator,
    causalConv1d,
)
from sbi_amd.neural_nets.embedding_nets.sc_embedding import (  # noqa: F401
    SpectralConv1d_SMM,
    SpectralConvEmbedding,
    VFT,
)
from sbi_amd.neural_nets.embedding_nets.transformer import (  # noqa: F401
    FullAttention,
    IdentityEncoder,
    MLP,
    MoeBlock,
    PositionalEncoder,
    RMSNorm,
    RotaryEncoder,
    TransformerBlock,
    TransformerEmbedding,
    ViTEmbeddings,
)
from sbi_amd.neural_nets.embedding_nets.resnet import (  # noqa: F401
    ResNetEmbedding1D,
    ResNetEmbedding2D,
    ResidualBLock,
    construct_simple_conv_net,
    construct_simple_fc_net,
    zero_pad,
)
