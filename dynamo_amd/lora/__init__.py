from .manager import LoRAAdapter, LoRABank, LoRAManager, lora_block_salt

__all__ = ["LoRAAdapter", "LoRABank", "LoRAManager", "lora_block_salt"]
