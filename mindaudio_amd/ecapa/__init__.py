"""ECAPA-TDNN recipes (mirror of examples/ECAPA-TDNN): speaker verification by cosine scoring, and the generation of augmented
training features (spec_augment, generate_train_data)."""
