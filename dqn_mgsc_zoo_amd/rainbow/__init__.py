"""Prioritized double-Q C51 agent: Rainbow's learning rule on the C51 network."""
