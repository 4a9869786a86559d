"""Fine-tuning of SAM on the HIP kernels (reference ``micro_sam/training``)."""
from .joint_sam_trainer import DiceBasedDistanceLoss, JointSamTrainer  # noqa: F401
from .label_transform import PerObjectDistanceTransform  # noqa: F401
from .sam_trainer import SamTrainer  # noqa: F401
from .semantic_sam_trainer import CustomDiceLoss, SemanticMapsSamTrainer, SemanticSamTrainer  # noqa: F401
from .trainable_sam import TrainableSAM  # noqa: F401
from .util import ConvertToSamInputs, ConvertToSemanticSamInputs, get_trainable_sam_model  # noqa: F401
