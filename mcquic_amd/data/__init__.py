from .transforms import AlignedCrop, TrainingInput, getEvalTransform, getTrainingPreprocess, getTrainingTransform

__all__ = ["AlignedCrop", "TrainingInput", "getEvalTransform", "getTrainingPreprocess", "getTrainingTransform"]
