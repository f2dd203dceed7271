"""ECAPA-TDNN recipes (mirror of examples/ECAPA-TDNN): speaker verification by cosine scoring."""
