from sbi_amd.neural_nets.factory import (build_score_matching_estimator, classifier_nn, likelihood_nn,  # noqa: F401
                                          posterior_flow_nn, posterior_nn, posterior_score_nn)
from sbi_amd.neural_nets.net_builders.estimator_configs import (MAFConfig, MAFRQSConfig, MDNConfig,  # noqa: F401
                                                                MixedConfig,
                                                                NSFConfig,
                                                                ResNetClassifierConfig, ZukoNSFConfig)
from sbi_amd.neural_nets.net_builders.flow import build_maf  # noqa: F401,E402
from sbi_amd.neural_nets.embedding_nets import (  # noqa: F401,E402
    CNNEmbedding,
    CausalCNNEmbedding,
    FCEmbedding,
    FullAttention,
    IdentityEncoder,
    LRU,
    LRUBlock,
    LRUEmbedding,
    MLP,
    MoeBlock,
    PermutationInvariantEmbedding,
    PositionalEncoder,
    RMSNorm,
    ResNetEmbedding1D,
    ResNetEmbedding2D,
    ResidualBLock,
    RotaryEncoder,
    SpectralConv1d_SMM,
    SpectralConvEmbedding,
    TransformerBlock,
    TransformerEmbedding,
    VFT,
    ViTEmbeddings,
    WaveNetSRLikeAggregator,
    calculate_filter_output_size,
    causalConv1d,
    construct_simple_conv_net,
    construct_simple_fc_net,
    get_new_cnn_output_size,
    zero_pad,
)
