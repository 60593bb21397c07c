"""MI355X-native conditional-SMC sweep for ParticleMDI (hot path of src/pmdi.jl).

The directory name `particlemdi.jl_amd` is not a Python identifier; load it
with `__graft_entry__.load_package()` which registers it as `particlemdi_jl_amd`.
"""
from ._lib import (  # noqa: F401
    ABI_VERSION, BLOCKSUM_GMAX, CATEGORICAL, EXPORTS, GAUSSIAN, KIND_BY_NAME, LIB_PATH, NEGBINOM, PARTDIST_GMAX,
    ClusterBatch, Comm, CsvWriter, Gibbs, format_float64, read_allocations, PmdiError, REFINE_GMAX, Sweeper, build, lib,
    STEP_ALIGN, STEP_BEGIN, STEP_FEATSEL, STEP_HYPERS, STEP_SWEEP,
)
from .pmdi import pmdi_pooled  # noqa: F401,E402    (not pmdi(): the name is the submodule's)
from .psm import (  # noqa: F401,E402
    AllocationRowScores, AllocationScores, BlockSimilarity, ConsensusMap, PsmAccumulator, PsmCounts, best_sampled_allocation,
    block_similarity, block_sums, consensus_map, refine_allocations,
    retained_iterations, row_scores, score_allocations, search_consensus_allocation, select_consensus_allocations, vi_log2_table,
)
from .partition import (  # noqa: F401,E402
    CredibleBall, PartitionDistances, credible_ball, minimise_expected_loss, partition_distances, refine_expected_loss)
from .datamap import (  # noqa: F401,E402
    ClusterProfiles, DataMap, cluster_profiles, column_moments, data_map, group_sums,
)
from .fusion import FusionAccumulator, FusionCounts, fused_consensus_allocations  # noqa: F401,E402
from .summary import (  # noqa: F401,E402
    PosteriorSummary, SummaryAccumulator, get_feature_select_probs, get_nclust, get_phi,
)
from .mixing import MixingAccumulator, MixingSummary  # noqa: F401,E402
from .predict import (  # noqa: F401,E402
    CoupledPredictiveCounts, PredictiveAccumulator, PredictiveCounts, check_new_rows, observed_masks)
from .loo import LooAccumulator, LooCounts  # noqa: F401,E402
from .density import DensityAccumulator, DensityResult  # noqa: F401,E402
from .agreement import AgreementAccumulator, AgreementSummary  # noqa: F401,E402
from .relabel import (  # noqa: F401,E402
    AllocationProbabilities, RelabelAccumulator, allocation_probabilities, assign_labels)
