"""sopro_amd: MI355X-native engine for the Sopro TTS synthesize/stream hot path.

``SoproTTS`` is the public name of the reference package (src/sopro/__init__.py:3-5); ``Watermark`` is what its ``watermark=``
keyword takes (``sopro_amd.watermark``), ``Silence`` what its ``silence=`` keyword takes (``sopro_amd.silence``), ``Denoise`` what its
``denoise=`` keyword takes and ``DenoiseReport`` what its ``report=`` sink receives (``sopro_amd.denoise``), ``SpeechCrop`` what its
``crop=`` keyword takes and ``CropReport`` what the sink receives for it (``sopro_amd.crop``); ``PitchTrack`` is what ``SoproTTS.pitch_track`` /
``SoproTTS.voice_pitch`` return and ``PitchParams`` what their ``params=`` keyword takes (``sopro_amd.f0``); ``VoiceMatch`` is what
``SoproTTS.voice_similarity`` returns and the ``similarity=`` sink receives, ``VoiceBank`` what ``SoproTTS.identify_voice`` searches and
``VoiceHit`` what it returns (``sopro_amd.voicematch``); ``TimedChunk`` and ``WordCue`` are what ``SoproTTS.stream_timed`` yields (``sopro_amd.align``).
Importing the package does not need a GPU; constructing an engine does (and raises otherwise).
"""
from .tts import SoproTTS  # noqa: F401
from .align import TimedChunk, WordCue  # noqa: F401
from .crop import CropReport, SpeechCrop  # noqa: F401
from .denoise import Denoise, DenoiseReport  # noqa: F401
from .f0 import PitchParams, PitchTrack  # noqa: F401
from .silence import Silence  # noqa: F401
from .voicematch import VoiceBank, VoiceHit, VoiceMatch  # noqa: F401
from .watermark import Watermark  # noqa: F401

__all__ = ["SoproTTS", "Watermark", "Silence", "Denoise", "DenoiseReport", "SpeechCrop", "CropReport", "TimedChunk", "WordCue",
           "PitchTrack", "PitchParams", "VoiceMatch", "VoiceBank", "VoiceHit"]
