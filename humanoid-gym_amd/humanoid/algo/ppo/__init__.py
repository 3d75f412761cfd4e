from .ppo import PPO
from .student_teacher import StudentTeacher
from .distillation import Distillation
from .rnd import RandomNetworkDistillation
from .on_policy_runner import OnPolicyRunner
from .actor_critic import ActorCritic
from .rollout_storage import RolloutStorage
