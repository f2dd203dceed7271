from .greedydecoder import Decoder, GreedyDecoder, MSGreedyDecoder  # noqa: F401
