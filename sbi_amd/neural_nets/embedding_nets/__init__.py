from sbi_amd.neural_nets.embedding_nets.fully_connected import FCEmbedding  # noqa: F401
from sbi_amd.neural_nets.embedding_nets.permutation_invariant import PermutationInvariantEmbedding  # noqa: F401
