from robopianist_amd.wrappers.canonical import CanonicalSpecWrapper
from robopianist_amd.wrappers.evaluation import MidiEvaluationWrapper
from robopianist_amd.wrappers.fingertip import FingertipActionWrapper
from robopianist_amd.wrappers.graphed import GraphedStepWrapper
from robopianist_amd.wrappers.hearing import AudioObservationWrapper
from robopianist_amd.wrappers.pixels import PixelWrapper
from robopianist_amd.wrappers.sound import PianoSoundVideoWrapper, PianoSoundWrapper

__all__ = ["CanonicalSpecWrapper", "MidiEvaluationWrapper", "GraphedStepWrapper", "PixelWrapper", "PianoSoundWrapper",
           "PianoSoundVideoWrapper", "AudioObservationWrapper", "FingertipActionWrapper"]
