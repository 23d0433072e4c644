"""QR-DQN agent (drop-in for dqn_zoo/qrdqn)."""
