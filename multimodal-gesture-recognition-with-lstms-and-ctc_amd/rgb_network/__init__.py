"""RGB network (reference rgb_network/): TimeDistributed CNN front-end -> 2x BiLSTM(512) + add -> Dense(22) -> CTC."""
