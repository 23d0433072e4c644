"""C51 agent (drop-in for dqn_zoo/c51)."""
