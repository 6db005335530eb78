def sayer(module_globals):
    """print for a module's progress lines: silent unless the module's VERBOSE is true at the time of the call."""
    def say(*args):
        if module_globals["VERBOSE"]:
            print(*args)

    return say
