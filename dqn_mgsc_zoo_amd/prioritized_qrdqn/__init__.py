"""Prioritized double-Q QR-DQN agent: Rainbow's learning rule on the QR-DQN network."""
