from .gae import gae
from .policy import ActorCritic
from .ppo import PPO, PPOConfig, allreduce_mean_, ppo_loss
from .population import (ArchPopulationPPO, DeployedPopulationPPO, PopulationPPO, deployed_population_for,
                         population_for)

__all__ = ["gae", "ActorCritic", "PPO", "PPOConfig", "ppo_loss", "allreduce_mean_", "PopulationPPO",
           "ArchPopulationPPO", "population_for", "DeployedPopulationPPO", "deployed_population_for"]
