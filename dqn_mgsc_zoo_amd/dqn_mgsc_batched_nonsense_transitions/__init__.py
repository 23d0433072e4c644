"""MGSC DQN agent that mixes nonsense transitions into its replay
(drop-in for dqn_zoo/dqn_mgsc_batched_nonsense_transitions)."""
